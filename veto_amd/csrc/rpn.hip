// RPNPostProcessor (pysgg/modeling/rpn/inference.py:13-183) for a whole batch and every pyramid level, on the device.
//
// A segment is one image x level.  Three launches (four in per-batch mode), whatever the number of images or levels; the levels'
// shapes and pointers travel as a descriptor table inside the kernel arguments, so one grid serves all of them.
//   rpn_select_kernel   one workgroup per segment, reading objectness / regression in place (NCHW; anchor (h W + w) A + a):
//                       the k = min(PRE_NMS_TOP_N, A H W) best anchors by (logit desc, anchor index asc; -0.0 and +0.0 are one
//                       logit and leave the selector as +0.0) -- radix select of the
//                       k-th largest logit over global memory, the candidates at or above it sorted in LDS --, then in that
//                       order BoxCoder.decode (box_coder.py:62-95), clip_to_image(remove_empty=False) and remove_small_boxes
//                       (boxlist_ops.py:35-49); the survivors go to the workspace, best first, with their count
//   nms_fixed_kernel    nms.hip: veto_nms on those fixed-capacity segments, at most POST_NMS_TOP_N survivors (skipped when
//                       NMS_THRESH <= 0, as boxlist_nms returns early)
//   rpn_batch_cut_kernel   per-batch mode only, one workgroup: the FPN_POST_NMS_TOP_N-th largest logit of the whole batch and how
//                       many of the logits equal to it each image may keep (ties: image, level, rank)
//   rpn_emit_kernel     one workgroup per image: select_over_all_levels (:156-183).  Per image: the survivors of all levels sorted
//                       by (logit desc, level asc, rank asc), the first FPN_POST_NMS_TOP_N emitted.  Per batch: the members of the
//                       batch-wide set in level-major, rank-ascending order.  One level: that level's survivors as they are.
// One workgroup per segment for the select, not a split over workgroups: a batch already has n_img x n_lvl segments in flight
// (60 for the VETO batch), the largest plane (91 200 logits, 356 KiB) stays in L2 across the five passes, and a split would need
// a hand-off between workgroups (an agent-scope release / acquire per pass, or a launch per pass) that costs more than the pass.
//
// The anchors it reads come from anchor_grid_kernel (below; AnchorGenerator.forward, rpn/anchor_generator.py:73-125): the grid of
// every level and the visibility plane of every image in one launch, one thread per anchor row.
#include "common.h"
#include "kernels.h"
#include "selection.h"

#pragma clang fp contract(off)   // BoxCoder.decode follows the reference operation for operation: NMS and min_size compare its results

namespace veto {

namespace {

struct RpnSelectLds {
  unsigned long long keys[kRpnSortCap];
  SelLds sel;
  int n_gt, n_eq;
};

__device__ __forceinline__ float float_unorder(uint32_t k) {   // inverse of float_order
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// f(position, value) for every element of x[0..N), in any order; 16-byte loads on the aligned body
template <class F>
__device__ __forceinline__ void visit_plane(const float* x, int N, F f) {
  const int tid = threadIdx.x;
  const int head = min(N, (int)(((16 - ((uintptr_t)x & 15)) & 15) >> 2));
  const int n4 = (N - head) >> 2;
  if (tid < head) f(tid, x[tid]);
  const float4* v = (const float4*)(x + head);
  for (int i = tid; i < n4; i += 256) {
    const float4 q = v[i];
    const int p = head + 4 * i;
    f(p, q.x);
    f(p + 1, q.y);
    f(p + 2, q.z);
    f(p + 3, q.w);
  }
  const int tail = head + 4 * n4 + tid;
  if (tail < N) f(tail, x[tail]);
}

__global__ __launch_bounds__(256) void rpn_select_kernel(RpnArgs a) {
  __shared__ RpnSelectLds L;
  const int seg = blockIdx.x, img = seg / a.n_lvl, tid = threadIdx.x;
  const RpnLevel& lv = a.lvl[seg - img * a.n_lvl];
  const int N = lv.N, HW = lv.HW, A = lv.A, k = lv.k;
  const float* logit = lv.objectness + (size_t)img * N;   // [A, H, W]: position p = a HW + hw is anchor hw A + a
  auto sort_key = [&](uint32_t key, uint32_t anchor) { return ((unsigned long long)(~key) << 32) | anchor; };
  int n;   // keys to sort; the first k of the sorted list are the selection
  if (k >= N) {
    visit_plane(logit, N, [&](int p, float v) {
      const int c = p / HW;
      L.keys[p] = sort_key(float_order(v), (uint32_t)(p - c * HW) * A + c);
    });
    n = N;
  } else {
    uint32_t T;
    int need;
    radix_select([&](auto f) { visit_plane(logit, N, [&](int, float v) { f(float_order(v)); }); }, k, L.sel, T, need);
    // every logit above T, and of those equal to T the `need` lowest anchors: all of them while they fit the sort
    const int n_gt = k - need, room = kRpnSortCap - n_gt;
    if (tid == 0) L.n_gt = L.n_eq = 0;
    __syncthreads();
    visit_plane(logit, N, [&](int p, float v) {
      const uint32_t key = float_order(v);
      if (key < T) return;
      const int c = p / HW;
      const unsigned long long sk = sort_key(key, (uint32_t)(p - c * HW) * A + c);
      if (key > T) {
        const int s = atomicAdd(&L.n_gt, 1);
        if (s < n_gt) L.keys[s] = sk;
      } else {
        const int s = atomicAdd(&L.n_eq, 1);
        if (s < room) L.keys[n_gt + s] = sk;
      }
    });
    __syncthreads();
    n = n_gt + L.n_eq;
    if (n > kRpnSortCap) {   // more ties at the cut than the sort holds: rank them in anchor order, thread t owns a range
      const int per = (N + 255) / 256, lo = min(N, tid * per), hi = min(N, lo + per);
      auto each = [&](auto f) {
        for (int i = lo; i < hi; ++i) f(float_order(logit[(size_t)(i % A) * HW + i / A]));
      };
      int r = equal_rank(each, T, L.sel);
      for (int i = lo; i < hi && r < need; ++i)
        if (float_order(logit[(size_t)(i % A) * HW + i / A]) == T) L.keys[n_gt + r++] = sort_key(T, (uint32_t)i);
      n = k;
    }
  }
  bitonic_sort(L.keys, n);   // (its first barrier is behind the writes above)
  const int kk = min(k, n);
  const float xmax = a.image_sizes[2 * img] - 1.f, ymax = a.image_sizes[2 * img + 1] - 1.f;
  const float* regression = lv.regression + (size_t)img * 4 * N;
  const size_t row0 = (size_t)seg * a.capacity;
  int total = 0;
  for (int base = 0; base < kk; base += 256) {
    const int t = base + tid;
    bool ok = false;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float x = 0.f;
    uint32_t anchor = 0;
    if (t < kk) {
      const unsigned long long sk = L.keys[t];
      anchor = (uint32_t)sk;
      x = float_unorder(~(uint32_t)(sk >> 32));
      const int c = anchor % A, hw = anchor / A;
      const float* reg = regression + (size_t)(4 * c) * HW + hw;
      const float4 p = ((const float4*)lv.anchors)[anchor];
      // BoxCoder.decode (box_coder.py:62-95), TO_REMOVE = 1
      const float w = (p.z - p.x) + 1.f, h = (p.w - p.y) + 1.f;
      const float cx = p.x + 0.5f * w, cy = p.y + 0.5f * h;
      const float dx = reg[0] / a.wx, dy = reg[HW] / a.wy;
      const float dw = fminf(reg[2 * (size_t)HW] / a.ww, a.xform_clip), dh = fminf(reg[3 * (size_t)HW] / a.wh, a.xform_clip);
      const float pcx = dx * w + cx, pcy = dy * h + cy;
      const float pw = expf(dw) * w, ph = expf(dh) * h;
      b.x = pcx - 0.5f * pw;
      b.y = pcy - 0.5f * ph;
      b.z = (pcx + 0.5f * pw) - 1.f;
      b.w = (pcy + 0.5f * ph) - 1.f;
      // clip_to_image(remove_empty=False): clamp_(min=0, max=size - 1)
      b.x = fminf(fmaxf(b.x, 0.f), xmax);
      b.y = fminf(fmaxf(b.y, 0.f), ymax);
      b.z = fminf(fmaxf(b.z, 0.f), xmax);
      b.w = fminf(fmaxf(b.w, 0.f), ymax);
      // remove_small_boxes: both sides of the xywh form >= min_size
      ok = (b.z - b.x) + 1.f >= a.min_size && (b.w - b.y) + 1.f >= a.min_size;
    }
    int cnt;
    const int pos = total + block_exclusive_scan(ok, L.sel.wave, &cnt);
    if (ok) {
      ((float4*)a.cand_box)[row0 + pos] = b;
      a.cand_logit[row0 + pos] = x;
      a.cand_anchor[row0 + pos] = (int32_t)anchor;
    }
    total += cnt;
  }
  if (tid == 0) a.live[seg] = total;
}

// survivors of a segment and the candidate row of its r-th survivor
__device__ __forceinline__ int seg_count(const RpnArgs& a, int seg) { return a.nms_on ? a.kept[seg] : a.live[seg]; }
__device__ __forceinline__ size_t seg_row(const RpnArgs& a, int seg, int r) {
  const size_t row0 = (size_t)seg * a.capacity;
  return row0 + (a.nms_on ? a.keep[row0 + r] : r);
}

constexpr int kCutImages = 1024;   // images of a per-batch cut (LDS counters)

__global__ __launch_bounds__(256) void rpn_batch_cut_kernel(RpnArgs a) {
  __shared__ SelLds sel;
  __shared__ int eq[kCutImages];
  const int tid = threadIdx.x, S = a.n_img * a.n_lvl;
  int mine = 0;
  for (int s = tid; s < S; s += 256) mine += seg_count(a, s);
  int total;
  block_exclusive_scan(mine, sel.wave, &total);
  if (total <= a.fpn_top_n) {
    if (tid == 0) a.cut[0] = 0;
    return;
  }
  auto each = [&](auto f) {
    for (int s = 0; s < S; ++s) {
      const int n = seg_count(a, s);
      for (int r = tid; r < n; r += 256) f(s / a.n_lvl, float_order(a.cand_logit[seg_row(a, s, r)]));
    }
  };
  uint32_t T;
  int need;
  radix_select([&](auto f) { each([&](int, uint32_t key) { f(key); }); }, a.fpn_top_n, sel, T, need);
  for (int i = tid; i < a.n_img; i += 256) eq[i] = 0;
  __syncthreads();
  each([&](int img, uint32_t key) {
    if (key == T) atomicAdd(&eq[img], 1);
  });
  __syncthreads();
  if (tid == 0) {
    a.cut[0] = 1;
    a.cut[1] = (int32_t)T;
    a.cut[2] = need;
    int before = 0;
    for (int i = 0; i < a.n_img; ++i) {
      a.cut[4 + i] = before;
      before += eq[i];
    }
  }
}

struct RpnEmitLds {
  unsigned long long keys[kRpnSortCap];
  SelLds sel;
  int first[kRpnMaxLevels + 1];   // concatenated position of each level's first survivor
};

__global__ __launch_bounds__(256) void rpn_emit_kernel(RpnArgs a) {
  __shared__ RpnEmitLds L;
  const int img = blockIdx.x, tid = threadIdx.x, seg0 = img * a.n_lvl;
  if (tid == 0) {
    int t = 0;
    for (int l = 0; l < a.n_lvl; ++l) {
      L.first[l] = t;
      t += seg_count(a, seg0 + l);
    }
    L.first[a.n_lvl] = t;
  }
  __syncthreads();
  const int total = L.first[a.n_lvl];
  const int out0 = a.out_off[img], capacity = a.out_off[img + 1] - out0;
  auto level_of = [&](int p) {
    int l = 0;
    while (p >= L.first[l + 1]) ++l;
    return l;
  };
  auto emit = [&](int p, int dst) {   // concatenated position p -> output row dst
    const int l = level_of(p);
    const size_t row = seg_row(a, seg0 + l, p - L.first[l]);
    ((float4*)a.boxes)[dst] = ((const float4*)a.cand_box)[row];
    a.objectness[dst] = 1.f / (1.f + expf(-a.cand_logit[row]));
    a.level[dst] = l;
    a.anchor_index[dst] = a.cand_anchor[row];
  };
  if (a.per_batch && a.n_lvl > 1) {   // inference.py:163-174: the members of the batch-wide set, in their own order
    const bool cut = a.cut[0] != 0;
    const uint32_t T = cut ? (uint32_t)a.cut[1] : 0u;
    const int need = a.cut[2], per = (total + 255) / 256, lo = min(total, tid * per), hi = min(total, lo + per);
    auto each = [&](auto f) {
      for (int p = lo; p < hi; ++p) {
        const int l = level_of(p);
        f(float_order(a.cand_logit[seg_row(a, seg0 + l, p - L.first[l])]));
      }
    };
    int r = cut ? a.cut[4 + img] + equal_rank(each, T, L.sel) : 0, mine = 0;
    const int r0 = r;
    each([&](uint32_t key) { mine += !cut || key > T || (key == T && r++ < need); });
    int fc;
    int pos = out0 + block_exclusive_scan(mine, L.sel.wave, &fc);
    if (fc > capacity) {   // the caller's rows do not hold the result: report the count, write nothing
      if (tid == 0) a.counts[img] = -fc;
      return;
    }
    r = r0;
    int p = lo;
    each([&](uint32_t key) {
      if (!cut || key > T || (key == T && r++ < need)) emit(p, pos++);
      ++p;
    });
    if (tid == 0) a.counts[img] = fc;
    return;
  }
  // :176-182 (and one level, where the order is already this one): (logit desc, level asc, rank asc), the first fpn_top_n
  const int fc = a.n_lvl > 1 ? min(a.fpn_top_n, total) : total;
  if (fc > capacity || total > kRpnSortCap) {   // (the ABI bounds total by the sort's size before anything is launched)
    if (tid == 0) a.counts[img] = -fc;
    return;
  }
  for (int p = tid; p < total; p += 256) {
    const int l = level_of(p);
    const uint32_t key = float_order(a.cand_logit[seg_row(a, seg0 + l, p - L.first[l])]);
    L.keys[p] = ((unsigned long long)(~key) << 32) | (uint32_t)p;
  }
  bitonic_sort(L.keys, total);
  for (int t = tid; t < fc; t += 256) emit((int)(uint32_t)L.keys[t], out0 + t);
  if (tid == 0) a.counts[img] = fc;
}

// AnchorGenerator.forward (anchor_generator.py:73-125): one thread per anchor row of the concatenated levels.  kGenerate: row
// (h W + w) A + a of a level is cell[a] + (w, h, w, h) * stride -- the shifts are integers below 2^24, exact in float32, so each
// coordinate is the one float32 addition the reference makes -- stored with one 16-byte store; otherwise the row is read from
// anchors_in.  Then, if asked for, the row's byte of every image's visibility plane (:100-106, in float32 like the reference's
// comparisons; straddle < 0: 1).  blockIdx.y owns kAnchorImages images; every y derives the row itself, y = 0 stores it.
// Store-bound: no LDS, nothing shared between threads.  With more than kAnchorImages images the generating instance derives a row
// once per y slice (a few integer operations, one 16-byte load from a table of A rows and four additions) to keep the slices
// independent; only the bytes of the plane are written more than once per row.
constexpr int kAnchorImages = 16;

template <bool kGenerate>
__global__ __launch_bounds__(256) void anchor_grid_kernel(AnchorArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  float4 p;
  if (kGenerate) {
    int l = 0;
    while (l + 1 < a.n_lvl && i >= a.lvl[l + 1].row0) ++l;
    const AnchorLevel& lv = a.lvl[l];
    const int r = i - lv.row0, cellpos = r / lv.A, c = r - cellpos * lv.A;
    const int h = cellpos / lv.W, w = cellpos - h * lv.W;
    const float sx = (float)(w * lv.stride), sy = (float)(h * lv.stride);
    const float4 q = ((const float4*)lv.cell)[c];
    p = make_float4(q.x + sx, q.y + sy, q.z + sx, q.w + sy);
    if (blockIdx.y == 0) ((float4*)a.anchors)[i] = p;
  } else {
    p = ((const float4*)a.anchors_in)[i];
  }
  if (!a.visibility) return;
  const int img0 = blockIdx.y * kAnchorImages, img1 = min(a.n_img, img0 + kAnchorImages);
  const float t = a.straddle;
  for (int img = img0; img < img1; ++img) {
    bool visible = true;
    if (t >= 0.f) {
      const float iw = a.image_sizes[2 * img], ih = a.image_sizes[2 * img + 1];
      visible = p.x >= -t && p.y >= -t && p.z < iw + t && p.w < ih + t;
    }
    a.visibility[(size_t)img * a.total + i] = visible ? 1 : 0;
  }
}

}  // namespace

int rpn_batch_cut_max_images() { return kCutImages; }

hipError_t launch_anchor_grid(const AnchorArgs& a, hipStream_t s) {
  const dim3 grid((a.total + 255) / 256, a.visibility ? (a.n_img + kAnchorImages - 1) / kAnchorImages : 1);
  if (a.anchors)
    VETO_LAUNCH(anchor_grid_kernel<true>, grid, dim3(256), 0, s, a);
  else
    VETO_LAUNCH(anchor_grid_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rpn_proposals(const RpnArgs& a, hipStream_t s) {
  const int n_seg = a.n_img * a.n_lvl;
  VETO_LAUNCH(rpn_select_kernel, dim3(n_seg), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.nms_on) {
    NmsFixedArgs n{};
    n.boxes = a.cand_box; n.scores = a.cand_logit; n.live = a.live;
    n.n_seg = n_seg; n.capacity = a.capacity; n.max_keep = a.post_top_n; n.thr = a.nms_thresh;
    n.keep = a.keep; n.counts = a.kept;
    e = launch_nms_fixed(n, s);
    if (e != hipSuccess) return e;
  }
  if (a.per_batch && a.n_lvl > 1) {
    VETO_LAUNCH(rpn_batch_cut_kernel, dim3(1), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  VETO_LAUNCH(rpn_emit_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
