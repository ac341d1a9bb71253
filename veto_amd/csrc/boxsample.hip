// sgdet training, the box head's sampler: FastRCNNSampling (pysgg/modeling/roi_heads/box_head/sampling.py:14-156) for a ragged
// batch.  The reference loops over the images on the host: a boxlist_iou matrix, Matcher, a clamp, a gather and two masked
// writes per image, and for subsample two nonzero / randperm pairs more.  Here the batch is one launch per stage.
//
//   box_match_kernel      grid (tile of 256 proposals, image).  The image's GT boxes (<= 256, 4 KiB) are staged in LDS; one thread
//                         owns one proposal and walks them in index order, so the N x M IoU matrix never exists.  The IoU is
//                         selection.h::boxlist_iou (FMA contraction off), bit-equal to the reference's fp32 matrix, and the
//                         strict `>` keeps the lowest GT index that reaches the maximum (max(dim=0) on the CPU).  Matcher
//                         (matcher.py:66-76): >= high -> the index, [low, high) -> -2, < low -> -1.  Labels in the convention
//                         of assign_label_to_proposals (every negative match -> 0, sampling.py:129) or of prepare_targets
//                         (-1 -> 0, -2 -> -1, :63-70); regression targets are BoxCoder.encode (box_coder.py:22-50) against GT
//                         max(matched, 0), operation for operation.
//   box_subsample_kernel  one workgroup per image: BalancedPositiveNegativeSampler (balanced_positive_negative_sampler.py:37-66)
//                         and the nonzero(pos | neg) of subsample (sampling.py:111-114).  Thread t owns a consecutive range of
//                         the image's proposals.  A class above its quota keeps the `quota` smallest (hash, proposal index), hash
//                         = the upper 32 bits of rng64(seed, image, class, proposal index): a uniformly random subset, as
//                         randperm(m)[:k] is as a set.  The survivors leave in ascending proposal order through one block scan.
#include "common.h"
#include "kernels.h"
#include "selection.h"

namespace veto {

namespace {

constexpr int kMaxGt = 256;       // GT boxes per image: the LDS stage
constexpr int kMaxPrp = 6144;     // proposals per image (the box decoder's segment limit): the class bytes of one image in LDS
constexpr int kMaxBatch = 2048;   // BATCH_SIZE_PER_IMAGE
constexpr int kTile = 256;

enum { kPickPos = 0, kPickNeg = 1 };
enum : uint8_t { kIgnore = 0, kPos = 1, kNeg = 2 };

__global__ __launch_bounds__(kTile) void box_match_kernel(BoxMatchArgs a) {
  __shared__ float4 s_gt[kMaxGt];
  const int img = blockIdx.y, tid = threadIdx.x;
  const int p0 = a.prp_off[img], n = a.prp_off[img + 1] - p0;
  const int t0 = a.tgt_off[img], m = a.tgt_off[img + 1] - t0;
  if ((int)blockIdx.x * kTile >= n || m <= 0 || m > kMaxGt) return;   // the ABI checks the host-side sizes; never index LDS past 256 rows
  const float4* gt = reinterpret_cast<const float4*>(a.tgt_boxes) + t0;
  for (int j = tid; j < m; j += kTile) s_gt[j] = gt[j];
  __syncthreads();
  const int i = blockIdx.x * kTile + tid;
  if (i >= n) return;
  const size_t row = (size_t)p0 + i;
  const float4 p = reinterpret_cast<const float4*>(a.prp_boxes)[row];
  const float pb[4] = {p.x, p.y, p.z, p.w};
  float best = 0.f;
  int arg = 0;
  for (int j = 0; j < m; ++j) {
    const float4 g = s_gt[j];
    const float gb[4] = {g.x, g.y, g.z, g.w};
    const float iou = boxlist_iou(gb, pb);
    if (j == 0 || iou > best) { best = iou; arg = j; }
  }
  int matched = arg;
  if (best < a.low) matched = -1;                        // Matcher.BELOW_LOW_THRESHOLD
  else if (best < a.high) matched = -2;                  // Matcher.BETWEEN_THRESHOLDS
  const int g = matched < 0 ? 0 : matched;               // clamp(min=0)
  int64_t label = a.tgt_labels[t0 + g];
  if (matched < 0) label = (a.mode == 1 && matched == -2) ? -1 : 0;
  a.matched[row] = matched;
  a.labels[row] = label;
  if (a.matched_rows) a.matched_rows[row] = t0 + g;
  if (a.targets) reinterpret_cast<float4*>(a.targets)[row] = encode_box(s_gt[g], p, a.wx, a.wy, a.ww, a.wh);
}

__global__ __launch_bounds__(256) void box_subsample_kernel(BoxSubsampleArgs a) {
  __shared__ uint8_t s_cls[kMaxPrp];
  __shared__ SelLds s_sel;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int p0 = a.prp_off[img], n = a.prp_off[img + 1] - p0;
  if (n <= 0 || n > kMaxPrp) {   // the ABI checks the host-side sizes; never index LDS past 6144 bytes
    if (tid == 0) a.counts[img] = 0;
    return;
  }
  const int64_t* lab = a.labels + p0;
  for (int i = tid; i < n; i += blockDim.x) {
    const int64_t l = lab[i];
    s_cls[i] = l >= 1 ? kPos : (l == 0 ? kNeg : kIgnore);
  }
  __syncthreads();
  const int chunk = (n + blockDim.x - 1) / blockDim.x;
  const int e0 = min(n, tid * chunk), e1 = min(n, e0 + chunk);
  int my_pos = 0, my_neg = 0;
  for (int e = e0; e < e1; ++e) {
    my_pos += s_cls[e] == kPos;
    my_neg += s_cls[e] == kNeg;
  }
  int m_pos, m_neg;
  (void)block_exclusive_scan(my_pos, s_sel.wave, &m_pos);
  (void)block_exclusive_scan(my_neg, s_sel.wave, &m_neg);
  const int num_pos = min(m_pos, a.num_pos);             // balanced_positive_negative_sampler.py:41-46
  const int num_neg = min(m_neg, a.batch - num_pos);

  // per class: the threshold key T, how many of the keys == T are kept, and this thread's rank among them
  uint32_t T[2] = {0, 0};
  int need[2] = {0, 0}, eq[2] = {0, 0};
  const int quota[2] = {num_pos, num_neg}, members[2] = {m_pos, m_neg};
  for (int c = 0; c < 2; ++c) {
    if (quota[c] <= 0 || quota[c] >= members[c]) continue;   // none or all: no draw (uniform over the block)
    const uint8_t cls = c == 0 ? kPos : kNeg;
    auto keys = [&](auto f) {
      for (int e = e0; e < e1; ++e)
        if (s_cls[e] == cls) f(~(uint32_t)(rng64(a.seed, img, c == 0 ? kPickPos : kPickNeg, (uint32_t)e) >> 32));
    };
    radix_select(keys, quota[c], s_sel, T[c], need[c]);
    eq[c] = equal_rank(keys, T[c], s_sel);
  }
  auto takes = [&](int e, int* eq_run) {
    const uint8_t cls = s_cls[e];
    if (cls == kIgnore) return false;
    const int c = cls == kPos ? 0 : 1;
    if (quota[c] <= 0) return false;
    if (quota[c] >= members[c]) return true;
    const uint32_t k = ~(uint32_t)(rng64(a.seed, img, c == 0 ? kPickPos : kPickNeg, (uint32_t)e) >> 32);
    if (k == T[c]) return eq_run[c]++ < need[c];
    return k > T[c];
  };
  int run[2] = {eq[0], eq[1]};
  int mine = 0;
  for (int e = e0; e < e1; ++e) mine += takes(e, run);
  int total;
  int slot = block_exclusive_scan(mine, s_sel.wave, &total);
  int64_t* out = a.sampled + (size_t)img * a.batch;
  run[0] = eq[0];
  run[1] = eq[1];
  for (int e = e0; e < e1; ++e)
    if (takes(e, run)) {
      if (slot < a.batch) out[slot] = e;
      ++slot;
    }
  if (tid == 0) a.counts[img] = min(total, a.batch);
}

}  // namespace

int box_match_max_gt() { return kMaxGt; }
int box_subsample_max_proposals() { return kMaxPrp; }
int box_subsample_max_batch() { return kMaxBatch; }

hipError_t launch_box_match(const BoxMatchArgs& a, int largest_prp, hipStream_t s) {
  const int tiles = (largest_prp + kTile - 1) / kTile;
  VETO_LAUNCH(box_match_kernel, dim3(tiles, a.n_img), dim3(kTile), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_box_subsample(const BoxSubsampleArgs& a, hipStream_t s) {
  VETO_LAUNCH(box_subsample_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
