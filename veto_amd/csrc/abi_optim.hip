// veto_optim_step (include/veto_amd.h): the host side of the fused optimizer (optim.hip) -- the argument checks, the layout of the
// tables the device reads, and the pinned staging buffers they are uploaded from.
#include "abi_internal.h"

#include <cmath>
#include <cstring>
#include <mutex>

extern "C" {

static_assert(VETO_OPTIM_CHUNK == kOptimChunk, "the header's chunk size is the kernels'");

// Does the tensor take part in this call?
static bool optim_active(const veto_optim_tensor_t& t) { return t.grad != nullptr && t.numel > 0; }

// the host fields every mode checks; *n_chunks: the rows of the chunk table
static int optim_check_shapes(const veto_optim_args_t* a, long long* n_chunks) {
  if (a->tensor_size != (int32_t)sizeof(veto_optim_tensor_t)) return fail(VETO_ERR_INVALID, "veto_optim_tensor_t size mismatch");
  if (a->n_tensors < 1 || a->n_tensors > kOptimMaxTensors) return fail(VETO_ERR_INVALID, "n_tensors %d outside 1..%d", a->n_tensors, kOptimMaxTensors);
  if (a->mode < VETO_OPTIM_NORMS || a->mode > VETO_OPTIM_CLIP_STEP) return fail(VETO_ERR_INVALID, "unknown mode %d", a->mode);
  if (!a->tensors) return fail(VETO_ERR_INVALID, "missing pointer: tensors");
  long long chunks = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    const veto_optim_tensor_t& t = a->tensors[i];
    if (t.numel < 0 || t.numel >= (1ll << 31)) return fail(VETO_ERR_INVALID, "tensor %d: numel %lld outside 0..2^31 - 1", i, (long long)t.numel);
    if (optim_active(t)) chunks += (t.numel + kOptimChunk - 1) / kOptimChunk;
  }
  if (chunks > kOptimMaxChunks) return fail(VETO_ERR_INVALID, "%lld chunks of %d elements, the limit is %d", chunks, kOptimChunk, kOptimMaxChunks);
  *n_chunks = chunks;
  return VETO_OK;
}

// The tables as the device reads them: [counter, 256 bytes][OptimTensor x n_tensors][OptimChunk x n_chunks], each part at a multiple
// of 256 bytes; this prefix of the workspace is what the call uploads.  Behind it: partial [n_chunks] and tensor_sq [n_tensors] doubles.
// (offsets, not pointers: the pinned staging copy of the prefix has the same layout)
struct OptimLayout { size_t tensors, chunks, upload, partial, tensor_sq, total; };
static OptimLayout optim_layout(int n_tensors, long long n_chunks) {
  OptimLayout l;
  Carver c{nullptr};
  c.take_offset(256);      // the counter
  l.tensors = c.take_offset((size_t)n_tensors * sizeof(OptimTensor));
  l.chunks = c.take_offset((size_t)n_chunks * sizeof(OptimChunk));
  l.upload = l.chunks + (size_t)n_chunks * sizeof(OptimChunk);      // (the upload ends with the table's last row, not with its region)
  l.partial = c.take_offset((size_t)n_chunks * 8);
  l.tensor_sq = c.take_offset((size_t)n_tensors * 8);
  l.total = c.off;
  return l;
}

size_t veto_optim_step_workspace_bytes(const veto_optim_args_t* a) {
  if (!a || a->struct_size != (int32_t)sizeof(veto_optim_args_t)) return 0;
  long long n_chunks = 0;
  if (optim_check_shapes(a, &n_chunks) != VETO_OK) return 0;
  return optim_layout(a->n_tensors, n_chunks).total;
}

// Pinned staging for the tables, one buffer per call in flight.  A buffer is taken again only when the event recorded behind the
// call that used it has completed, so rewriting it cannot reach a copy that has not run yet.
struct OptimStage { void* host = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; int device = -1; };
static std::mutex g_optim_mutex;
static std::vector<OptimStage> g_optim_stages;
constexpr size_t kOptimMaxStages = 256;

static int optim_stage_acquire(size_t need, int device, OptimStage** out) {
  OptimStage* idle_small = nullptr;
  for (OptimStage& st : g_optim_stages) {
    if (st.device != device || hipEventQuery(st.done) != hipSuccess) continue;
    if (st.bytes >= need) { *out = &st; return VETO_OK; }
    idle_small = &st;
  }
  (void)hipGetLastError();   // hipErrorNotReady of a busy buffer is no error
  OptimStage* st = idle_small;
  if (!st && g_optim_stages.size() >= kOptimMaxStages) {   // 256 calls in flight on this device: wait for the oldest buffer
    for (OptimStage& o : g_optim_stages)
      if (o.device == device) { st = &o; break; }
    if (!st) return fail(VETO_ERR_HIP, "no staging buffer left for device %d", device);
    HIP_TRY(hipEventSynchronize(st->done));
    if (st->bytes >= need) { *out = st; return VETO_OK; }
  }
  if (st) {   // idle and too small: the parameter set grew
    HIP_TRY(hipHostFree(st->host));
    st->host = nullptr; st->bytes = 0;
  } else {
    g_optim_stages.emplace_back();
    st = &g_optim_stages.back();
    st->device = device;
    HIP_TRY(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
  }
  size_t bytes = 64 << 10;
  while (bytes < need) bytes *= 2;
  HIP_TRY(hipHostMalloc(&st->host, bytes, hipHostMallocDefault));
  st->bytes = bytes;
  *out = st;
  return VETO_OK;
}

int veto_optim_step(void* stream, const veto_optim_args_t* a, void* workspace, size_t workspace_bytes) {
  CHECK_STRUCT(veto_optim_args_t, a);
  long long n_chunks = 0;
  ABI_TRY(optim_check_shapes(a, &n_chunks));
  const bool norms = a->mode != VETO_OPTIM_STEP, steps = a->mode == VETO_OPTIM_STEP || a->mode == VETO_OPTIM_CLIP_STEP;
  const bool clips = a->mode == VETO_OPTIM_CLIP || a->mode == VETO_OPTIM_CLIP_STEP;
  if (clips && !(a->max_norm > 0.0)) return fail(VETO_ERR_INVALID, "max_norm %g must be > 0 in a mode that clips", a->max_norm);
  if (norms && (!a->norms || !a->total_norm || !a->coef)) return fail(VETO_ERR_INVALID, "missing pointer: norms, total_norm and coef are required");
  if (norms && (((uintptr_t)a->norms | (uintptr_t)a->total_norm | (uintptr_t)a->coef) & 3) != 0) return fail(VETO_ERR_INVALID, "misaligned norms, total_norm or coef");
  for (int i = 0; i < a->n_tensors; ++i) {
    const veto_optim_tensor_t& t = a->tensors[i];
    if (!optim_active(t)) continue;
    if (((uintptr_t)t.grad & 3) != 0) return fail(VETO_ERR_INVALID, "tensor %d: misaligned grad", i);
    if (!steps) continue;
    if (t.step < 1) return fail(VETO_ERR_INVALID, "tensor %d: step %lld must be >= 1 (the count including this update)", i, (long long)t.step);
    if (!t.param || !t.exp_avg || !t.exp_avg_sq) return fail(VETO_ERR_INVALID, "tensor %d: missing pointer: param, exp_avg and exp_avg_sq are required", i);
    if ((((uintptr_t)t.param | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 3) != 0) return fail(VETO_ERR_INVALID, "tensor %d: misaligned param, exp_avg or exp_avg_sq", i);
    if (!(t.lr >= 0.0)) return fail(VETO_ERR_INVALID, "tensor %d: lr %g must be >= 0", i, t.lr);
    if (!(t.eps >= 0.0)) return fail(VETO_ERR_INVALID, "tensor %d: eps %g must be >= 0", i, t.eps);
    if (!(t.weight_decay >= 0.0)) return fail(VETO_ERR_INVALID, "tensor %d: weight_decay %g must be >= 0", i, t.weight_decay);
    if (!(t.beta1 >= 0.0 && t.beta1 < 1.0)) return fail(VETO_ERR_INVALID, "tensor %d: beta1 %g outside [0, 1)", i, t.beta1);
    if (!(t.beta2 >= 0.0 && t.beta2 < 1.0)) return fail(VETO_ERR_INVALID, "tensor %d: beta2 %g outside [0, 1)", i, t.beta2);
  }
  const OptimLayout lay = optim_layout(a->n_tensors, n_chunks);
  ABI_TRY(check_workspace(workspace, workspace_bytes, lay.total, true));

  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g_optim_mutex);
  OptimStage* st = nullptr;
  ABI_TRY(optim_stage_acquire(lay.upload, device, &st));
  char* host = (char*)st->host;
  memset(host, 0, 256);   // the counter
  OptimTensor* rows = (OptimTensor*)(host + lay.tensors);
  OptimChunk* chunk_rows = (OptimChunk*)(host + lay.chunks);
  int next = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    const veto_optim_tensor_t& t = a->tensors[i];
    OptimTensor r{};
    r.numel = (int)t.numel; r.chunk0 = next;
    if (optim_active(t)) {
      r.p = t.param; r.g = t.grad; r.m = t.exp_avg; r.v = t.exp_avg_sq;
      r.n_chunks = (int)((t.numel + kOptimChunk - 1) / kOptimChunk);
      for (int k = 0; k < r.n_chunks; ++k) chunk_rows[next++] = OptimChunk{i, k};
      if (steps) {
        const double bc1 = 1.0 - pow(t.beta1, (double)t.step), bc2 = 1.0 - pow(t.beta2, (double)t.step);
        r.wd = (float)t.weight_decay; r.beta1 = (float)t.beta1; r.omb1 = (float)(1.0 - t.beta1);
        r.beta2 = (float)t.beta2; r.omb2 = (float)(1.0 - t.beta2); r.eps = (float)t.eps;
        r.step_size = (float)(t.lr / bc1); r.bc2_sqrt = (float)sqrt(bc2);
      }
    }
    rows[i] = r;
  }
  char* ws = (char*)workspace;
  OptimArgs p{};
  p.tensors = (const OptimTensor*)(ws + lay.tensors); p.chunks = (const OptimChunk*)(ws + lay.chunks); p.counter = (unsigned*)ws;
  p.partial = (double*)(ws + lay.partial); p.tensor_sq = (double*)(ws + lay.tensor_sq);
  p.n_tensors = a->n_tensors; p.n_chunks = (int)n_chunks; p.max_norm = a->max_norm;
  p.norms = a->norms; p.total = a->total_norm; p.coef = a->coef;
  HIP_TRY(hipMemcpyAsync(ws, host, lay.upload, hipMemcpyHostToDevice, (hipStream_t)stream));
  const hipError_t e = launch_optim(p, norms, a->mode == VETO_OPTIM_CLIP ? 1 : steps ? 2 : 0, clips, (hipStream_t)stream);
  HIP_TRY(hipEventRecord(st->done, (hipStream_t)stream));   // behind the copy, whatever became of the launches
  if (e != hipSuccess) return fail(VETO_ERR_HIP, "launch_optim failed: %s", hipGetErrorString(e));
  return VETO_OK;
}

}  // extern "C"
