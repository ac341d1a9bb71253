// Training-time losses and MEET expert sampling (the parts named there).
//   * weighted cross entropy with mean reduction, nn.CrossEntropyLoss(weight=w): the relation loss of
//     VETOPredictor (roi_relation_predictors.py:4067-4068,4133; BETA_LOSS class-balanced weights :4057-4066) and,
//     unweighted on a row subset with remapped labels, the per-group losses of Ensemble.forward (:3842-3846).
//     loss = sum_i w[y_i] (logsumexp(z_i) - z_i[y_i]) / sum_i w[y_i]; d loss / d z_i = w[y_i] (softmax(z_i) - e_{y_i}) / sum w.
//     One wave per row for the row maximum and the log of the shifted sum (kept apart: the result does not depend on the
//     logits' offset), a fixed-order double-precision fold (deterministic), one wave per row for the gradient.
//   * the expert sampling loop of VETOPredictor_MEET.forward (:3940-3969), which the reference runs in Python with one
//     .item() per relation: here one wave walks the relations in order, consuming the SAME random stream (raw MT19937
//     words of Python's `random`, prepared by the host: random() = two words, randint = rejection on the top bits),
//     and appends each relation to its groups; a second kernel remaps the labels per group (:3812-3821).
#include "common.h"
#include "kernels.h"

namespace veto {

namespace {

// Cross entropy is invariant under a shift of a row's logits, and so is this kernel: the row maximum mx and log_sum = logf(sum exp(z - mx))
// are kept apart, and both the loss term and the gradient's exponent are formed as (z - mx) - log_sum.  (One float holding
// mx + log_sum is rounded at the size of mx: ulp(mx) / 2 of absolute error in every exponent, 3.5e-4 of the gradient at logits
// near 1e4.)  Every rounding after z - mx happens at the size of the row's spread, whatever its offset.
__global__ __launch_bounds__(256) void ce_rows_kernel(CeLossArgs a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= a.n) return;
  const long r = a.rows ? a.rows[i] : i;
  const float* z = a.logits + r * a.ld;
  float mx = -INFINITY;
  for (int c = lane; c < a.C; c += 64) mx = fmaxf(mx, z[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int c = lane; c < a.C; c += 64) sum += expf(z[c] - mx);
  sum = wave_sum(sum);
  if (lane == 0) {
    // a NEGATIVE label -- nn.CrossEntropyLoss's ignore_index (-100) -- is an ignored row: weight 0.  A label >= C is a bug in the
    // caller's class mapping (torch raises): the row poisons the loss with NaN instead of silently dropping out of it.
    const long yl = a.labels[i];
    const bool valid = yl >= 0 && yl < a.C, bad = yl >= a.C;
    const int y = valid ? (int)yl : 0;
    const float log_sum = logf(sum);
    const float w = valid ? (a.weight ? a.weight[y] : 1.f) : 0.f;
    a.log_sum[i] = log_sum;
    a.nll_w[i] = bad ? __builtin_nanf("") : valid ? w * (log_sum - (z[y] - mx)) : 0.f;
    a.w_row[i] = w;
  }
}

// loss = sum nll_w / sum w, rows folded in index order in double precision (one workgroup, deterministic)
__global__ __launch_bounds__(256) void ce_reduce_kernel(CeLossArgs a) {
  __shared__ double s_num[256], s_den[256];
  const int tid = threadIdx.x;
  const int per = (a.n + 255) / 256;
  double num = 0.0, den = 0.0;
  for (int i = tid * per; i < (tid + 1) * per && i < a.n; ++i) { num += (double)a.nll_w[i]; den += (double)a.w_row[i]; }
  s_num[tid] = num;
  s_den[tid] = den;
  __syncthreads();
  if (tid == 0) {
    double n2 = 0.0, d2 = 0.0;
    for (int t = 0; t < 256; ++t) { n2 += s_num[t]; d2 += s_den[t]; }
    a.loss[0] = (float)(n2 / d2);
    a.inv_wsum[0] = (float)(1.0 / d2);
  }
}

// d loss / d z = w_row / sum w (softmax(z) - e_y), the softmax as expf((z - mx) - log_sum) with mx found again (one more pass over a
// row of at most a few hundred values, which keeps the workspace layout).  An ignored row's gradient is exactly 0 whatever the weight
// sum -- with every label negative 1 / sum w is inf, and 0 * inf would be NaN; torch gives 0 there.  A valid row of weight 0 under a
// weight sum of 0 is NaN, as in torch.
__global__ __launch_bounds__(256) void ce_grad_kernel(CeLossArgs a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= a.n) return;
  const long r = a.rows ? a.rows[i] : i;
  const float* z = a.logits + r * a.ld;
  const long yl = a.labels[i];
  const int y = (yl >= 0 && yl < a.C) ? (int)yl : -1;
  float* g = a.grad + (size_t)i * a.C;
  if (yl < 0) {
    for (int c = lane; c < a.C; c += 64) g[c] = 0.f;
    return;
  }
  float mx = -INFINITY;
  for (int c = lane; c < a.C; c += 64) mx = fmaxf(mx, z[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  // a label >= C made the loss NaN (above); its gradient row is NaN too, so that an optimizer step cannot proceed on a loss that
  // never was one (torch raises in this case)
  const float scale = yl >= a.C ? __builtin_nanf("") : a.w_row[i] * a.inv_wsum[0], log_sum = a.log_sum[i];
  for (int c = lane; c < a.C; c += 64) g[c] = (expf((z[c] - mx) - log_sum) - (c == y ? 1.f : 0.f)) * scale;
}

// ---- MEET expert sampling --------------------------------------------------------------------------------
// Python's random on raw words: random() = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53; randint(0, G-1) = rejection
// sampling on the top bit_length(G) bits of one word per attempt (CPython _randbelow_with_getrandbits).
__global__ void meet_sample_kernel(MeetSampleArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int pos = 0;
  const int G = a.n_groups;
  int kbits = 0;
  while ((G >> kbits) != 0) ++kbits;
  for (int k = 0; k < G; ++k) a.counts[k] = 0;
  int overflow = 0;
  for (int i = 0; i < a.n; ++i) {
    const int lab = (int)a.labels[i];
    int upto;         // the relation goes to groups 0 .. upto-1, or to the single group `single`
    int single = -1;
    if (lab == 0) {
      if (pos >= a.n_words) { overflow = 1; break; }
      unsigned r = a.words[pos++] >> (32 - kbits);
      while (r >= (unsigned)G) {
        if (pos >= a.n_words) { overflow = 1; break; }
        r = a.words[pos++] >> (32 - kbits);
      }
      if (overflow) break;
      single = (int)r;
      upto = 0;
    } else {
      if (pos + 2 > a.n_words) { overflow = 1; break; }
      const unsigned w0 = a.words[pos] >> 5, w1 = a.words[pos + 1] >> 6;
      pos += 2;
      const double u = ((double)w0 * 67108864.0 + (double)w1) * (1.0 / 9007199254740992.0);
      const int g = a.incre[lab];
      upto = 0;
      for (int act = G; act >= 1; --act)
        if (u <= a.rates[(size_t)(act - 1) * a.n_cls + lab] || act < g) { upto = act; break; }
    }
    if (single >= 0) {
      a.chosen[(size_t)single * a.n + a.counts[single]++] = i;
    } else {
      for (int k = 0; k < upto; ++k) a.chosen[(size_t)k * a.n + a.counts[k]++] = i;
    }
  }
  a.words_used[0] = overflow ? -1 : pos;
}

// group-local labels of the chosen rows (:3812-3821): own classes -> 1.., other foreground -> size + 1, background 0
__global__ __launch_bounds__(256) void meet_labels_kernel(MeetSampleArgs a) {
  const int k = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.counts[k]) return;
  const int lab = (int)a.labels[a.chosen[(size_t)k * a.n + i]];
  int out = 0;
  if (lab != 0) out = a.incre[lab] == k + 1 ? a.pos_in_group[lab] : a.group_size[k] + 1;
  a.group_labels[(size_t)k * a.n + i] = out;
}

// ---- the same sampling, parallel but for the rand_insert word chain ------------------------------------------------
// What a relation does depends on the word it starts at, and that is a prefix sum of what the relations before it consumed:
//   rand_choose   every relation consumes two words: relation i starts at 2 i;
//   all_include   a foreground relation consumes two, a background none: 2 x (foreground relations in front of i);
//   rand_insert   a background consumes words up to its first accepted one, so the start of relation i+1 depends on the WORDS:
//                 pos' = fg ? pos + 2 : next_accepted(pos) + 1.  That chain stays serial, but it runs on two bit masks (one bit per
//                 relation: foreground; one bit per word: randint accepts it) that a parallel pass makes first; one wave walks it
//                 with every lane holding the same state, the masks in registers (lane l of a window register holds mask word
//                 64 w + l, fetched with a lane read), so that no load sits on the dependent chain.
// Then every relation decides in parallel from its own word(s) which groups lo..hi-1 it joins, and a stable compaction (ballot
// ranks inside a wave, wave counts inside a tile, tile counts in front of a tile; no atomics) writes the per-group lists in
// ascending relation order.  meet_labels_kernel, unchanged, comes last.
constexpr int kMeetTile = 1024, kMeetChunk = 64, kMeetWindow = 64 * kMeetChunk;
using u64 = unsigned long long;

__device__ __forceinline__ int meet_kbits(int G) {
  int kbits = 0;
  while ((G >> kbits) != 0) ++kbits;
  return kbits;
}

__device__ __forceinline__ double meet_uniform(unsigned a, unsigned b) {      // random.random() on the two raw words a, b
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(256) void meet_mask_kernel(MeetParallelArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;      // lane 0 of a wave: the first bit of one mask word
  const int lane = threadIdx.x & 63;
  const u64 fg = __ballot(idx < a.s.n && a.s.labels[idx] != 0);
  if (lane == 0 && idx < a.s.n) a.fg_mask[idx >> 6] = fg;
  if (a.mode != MEET_RAND_INSERT) return;
  const int shift = 32 - meet_kbits(a.s.n_groups);
  const u64 acc = __ballot(idx < a.s.n_words && (a.s.words[idx] >> shift) < (unsigned)a.s.n_groups);
  if (lane == 0 && idx < a.s.n_words) a.acc_mask[idx >> 6] = acc;      // (the bits behind n_words are 0: never accepted)
}

__device__ __forceinline__ u64 meet_mask_word(const u64* m, long n_mask, long idx) { return idx < n_mask ? m[idx] : 0ull; }

__device__ __forceinline__ u64 meet_lane_read(u64 v, int src) {      // v of lane src (the same src in every lane)
  src = __builtin_amdgcn_readfirstlane(src);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}

// one wave.  words_used, and what the decision needs to find each relation's words (MeetParallelArgs::pos)
__global__ __launch_bounds__(64) void meet_position_kernel(MeetParallelArgs a) {
  const int lane = threadIdx.x;
  const int n = a.s.n;
  const unsigned n_words = (unsigned)a.s.n_words;
  const long nF = ((long)n + 63) >> 6;
  if (a.mode == MEET_RAND_CHOOSE) {
    if (lane == 0) a.s.words_used[0] = 2ll * n <= (long long)n_words ? 2 * n : -1;
    return;
  }
  if (a.mode == MEET_ALL_INCLUDE) {      // exclusive prefix count of the foreground bits, 64 mask words per step
    long long carry = 0;
    for (long base = 0; base < nF; base += 64) {
      const int c = __popcll(meet_mask_word(a.fg_mask, nF, base + lane));
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      if (base + lane < nF) a.pos[base + lane] = (int)(carry + incl - c);      // (< n)
      carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) a.s.words_used[0] = 2 * carry <= (long long)n_words ? (int)(2 * carry) : -1;
    return;
  }
  // rand_insert: the chain.  Every lane holds the same pos / cur / nxt; r0, r1, r2 are the mask words of windows c, c+1, c+2 (the
  // third was asked for a whole window ago: nobody waits for it)
  const long nA = ((long)n_words + 63) >> 6;
  int c = 0;
  u64 r0 = meet_mask_word(a.acc_mask, nA, lane), r1 = meet_mask_word(a.acc_mask, nA, 64 + lane), r2 = meet_mask_word(a.acc_mask, nA, 128 + lane);
  int curidx = 0;                                   // cur = mask word curidx, nxt = mask word curidx + 1
  u64 cur = meet_lane_read(r0, 0), nxt = meet_lane_read(r0, 1);
  unsigned pos = 0;
  bool overflow = false;
  u64 fg_next = meet_mask_word(a.fg_mask, nF, 0);
  for (long fw = 0; fw < nF && !overflow; ++fw) {
    const u64 fg = fg_next;
    fg_next = meet_mask_word(a.fg_mask, nF, fw + 1);      // (asked for 64 relations before it is looked at)
    const int cnt = (int)(n - fw * 64 < 64 ? n - fw * 64 : 64);
    int mine = 0;
    int b = 0;
    while (b < cnt) {      // run by run: a lone wave pays per instruction, so a foreground run is one addition, a background one ctz
      const u64 rest = fg >> b;
      if (rest & 1ull) {
        const u64 stop = ~rest;
        int run = stop != 0 ? __builtin_ctzll(stop) : 64;
        run = run < cnt - b ? run : cnt - b;
        if ((u64)pos + 2ull * run > n_words) { overflow = true; break; }
        if (lane >= b && lane < b + run) mine = (int)pos + 2 * (lane - b);
        pos += 2u * run;
        b += run;
        continue;
      }
      const int run = rest != 0 ? __builtin_ctzll(rest) : 64;
      const int end = b + run < cnt ? b + run : cnt;
      while (b < end) {
        if (pos >= n_words) { overflow = true; break; }
        const int w = (int)(pos >> 6);
        while (curidx < w) {
          ++curidx;
          cur = nxt;
          const int want = curidx + 1;
          if ((want >> 6) > c + 1) {      // (want grows by one per step: one shift is enough)
            r0 = r1; r1 = r2; ++c;
            r2 = meet_mask_word(a.acc_mask, nA, (long)(c + 2) * 64 + lane);
          }
          nxt = meet_lane_read((want >> 6) == c ? r0 : r1, want & 63);
        }
        u64 m = cur >> (pos & 63u);      // the accepted words from pos to the end of mask word w: one per background relation
        while (m != 0 && b < end) {
          const int t = __builtin_ctzll(m);
          const unsigned rec = pos + (unsigned)t;      // (< n_words: the mask has no bit behind the block)
          if (lane == b) mine = (int)rec;
          ++b;
          pos = rec + 1u;
          m = (m >> t) >> 1;
        }
        if (b < end) pos = ((unsigned)w + 1u) << 6;      // nothing accepted in the rest of this mask word
      }
      if (overflow) break;
    }
    if (lane < cnt) a.pos[fw * 64 + lane] = mine;      // (after an overflow: unspecified, and the decision checks every position)
  }
  if (lane == 0) a.s.words_used[0] = overflow ? -1 : (int)pos;
}

__device__ __forceinline__ bool meet_member(int lo, int hi, int k) { return lo <= k && k < hi; }

// per-wave rows of each group (lane k: group k) into s_cnt[wave][k]
__device__ __forceinline__ void meet_wave_counts(int lo, int hi, int G, int (*s_cnt)[64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int mine = 0;
  for (int k = 0; k < G; ++k) {
    const int c = __popcll(__ballot(meet_member(lo, hi, k)));
    if (lane == k) mine = c;
  }
  s_cnt[wave][lane] = mine;
}

__global__ __launch_bounds__(kMeetTile) void meet_decide_kernel(MeetParallelArgs a) {
  __shared__ int s_cnt[kMeetTile / 64][64];
  const int G = a.s.n_groups, n = a.s.n;
  const long long n_words = a.s.n_words;
  const long i = (long)blockIdx.x * kMeetTile + threadIdx.x;
  int lo = 0, hi = 0;
  if (i < n) {
    const long lab = a.s.labels[i];
    long long p;      // the relation's first word (rand_insert background: its accepted word)
    if (a.mode == MEET_RAND_INSERT) p = a.pos[i];
    else if (a.mode == MEET_RAND_CHOOSE) p = 2ll * i;
    else p = 2ll * (a.pos[i >> 6] + __popcll(a.fg_mask[i >> 6] & ((1ull << (i & 63)) - 1ull)));
    if (lab != 0) {
      if (lab > 0 && lab < a.s.n_cls && p >= 0 && p + 2 <= n_words) {      // (an overflowing call: no row, nothing read out of bounds)
        const double u = meet_uniform(a.s.words[p], a.s.words[p + 1]);
        const int g = a.s.incre[lab];
        for (int act = G; act >= 1; --act)
          if (u <= a.s.rates[(size_t)(act - 1) * a.s.n_cls + lab] || act < g) { hi = act; break; }
      }
    } else if (a.mode == MEET_RAND_INSERT) {
      if (p >= 0 && p < n_words) {
        const unsigned r = a.s.words[p] >> (32 - meet_kbits(G));
        if (r < (unsigned)G) { lo = (int)r; hi = lo + 1; }
      }
    } else if (a.mode == MEET_RAND_CHOOSE) {
      if (p + 2 <= n_words && meet_uniform(a.s.words[p], a.s.words[p + 1]) >= 0.4) hi = G;
    } else {
      hi = G;
    }
    a.span[i] = (uint16_t)(lo | (hi << 8));
  }
  meet_wave_counts(lo, hi, G, s_cnt);
  __syncthreads();
  if (threadIdx.x < 64) {
    int sum = 0;
    for (int w = 0; w < kMeetTile / 64; ++w) sum += s_cnt[w][threadIdx.x];
    a.tile_count[(size_t)blockIdx.x * 64 + threadIdx.x] = sum;
  }
}

// one wave, lane k = group k: tile counts -> rows in front of each tile, and the list lengths
__global__ __launch_bounds__(64) void meet_offsets_kernel(MeetParallelArgs a, long tiles) {
  const int k = threadIdx.x;
  int run = 0;
  for (long t = 0; t < tiles; ++t) {
    const int c = a.tile_count[t * 64 + k];
    a.tile_count[t * 64 + k] = run;
    run += c;
  }
  if (k < a.s.n_groups) a.s.counts[k] = run;
}

__global__ __launch_bounds__(kMeetTile) void meet_scatter_kernel(MeetParallelArgs a) {
  __shared__ int s_cnt[kMeetTile / 64][64];
  const int G = a.s.n_groups, n = a.s.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * kMeetTile + threadIdx.x;
  const int sp = i < n ? a.span[i] : 0;
  const int lo = sp & 255, hi = sp >> 8;
  meet_wave_counts(lo, hi, G, s_cnt);
  __syncthreads();
  int base = a.tile_count[(size_t)blockIdx.x * 64 + lane];      // lane k: where this wave's rows of group k start
  for (int w = 0; w < wave; ++w) base += s_cnt[w][lane];
  for (int k = 0; k < G; ++k) {
    const bool in = meet_member(lo, hi, k);
    const u64 m = __ballot(in);
    const int at = __shfl(base, k, 64);
    if (in) a.s.chosen[(size_t)k * n + at + __popcll(m & ((1ull << lane) - 1ull))] = i;
  }
}

}  // namespace

int meet_parallel_tile() { return kMeetTile; }
int meet_parallel_window() { return kMeetWindow; }
int meet_parallel_chunk() { return kMeetChunk; }

hipError_t launch_meet_sample_parallel(const MeetParallelArgs& a, hipStream_t s) {
  const long span = a.mode == MEET_RAND_INSERT && a.s.n_words > a.s.n ? a.s.n_words : a.s.n;
  const long tiles = meet_parallel_tiles(a.s.n);
  hipError_t e;
  VETO_LAUNCH(meet_mask_kernel, dim3((unsigned)((span + 255) / 256)), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(meet_position_kernel, dim3(1), dim3(64), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(meet_decide_kernel, dim3((unsigned)tiles), dim3(kMeetTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(meet_offsets_kernel, dim3(1), dim3(64), 0, s, a, tiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(meet_scatter_kernel, dim3((unsigned)tiles), dim3(kMeetTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(meet_labels_kernel, dim3((a.s.n + 255) / 256, a.s.n_groups), dim3(256), 0, s, a.s);
  return hipGetLastError();
}

hipError_t launch_ce_loss(const CeLossArgs& a, hipStream_t s) {
  VETO_LAUNCH(ce_rows_kernel, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  VETO_LAUNCH(ce_reduce_kernel, dim3(1), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.grad) {
    VETO_LAUNCH(ce_grad_kernel, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_meet_sample(const MeetSampleArgs& a, hipStream_t s) {
  VETO_LAUNCH(meet_sample_kernel, dim3(1), dim3(64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  VETO_LAUNCH(meet_labels_kernel, dim3((a.n + 255) / 256, a.n_groups), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
