// C-ABI of the optimiser step (include/nar_fs2.h ns_opt_*): clip_grad_norm_, Adam.step() under ScheduledOptim and zero_grad()
// (train.py:91-95, model/optimizer.py:10-15,24,28).  No handle: the chunk table, the workspace, the two state arenas and the norm
// record all belong to the caller.  The planner and the table builder are host-only; every argument of the four launching calls is
// validated before the first HIP call.
#include "../../include/nar_fs2.h"
#include "host_core.h"

using namespace ns;

static_assert(sizeof(ns_opt_tensor) == sizeof(OptTensor) && sizeof(ns_opt_tensor) == 40, "ns_opt_tensor layout");
static_assert(sizeof(ns_opt_record) == sizeof(OptRecord) && sizeof(ns_opt_record) == 16, "ns_opt_record layout");
static_assert(sizeof(ns_opt_hyper) == sizeof(OptHyper) && sizeof(ns_opt_hyper) == 56, "ns_opt_hyper layout");
static_assert(sizeof(ns_opt_plan) == 40, "ns_opt_plan layout");
static_assert(NS_OPT_CHUNK == OPT_CHUNK, "chunk size");

namespace {
// chunks and padded state floats of one tensor
inline long long chunks_of(long long numel) { return numel <= 0 ? 1 : (numel + OPT_CHUNK - 1) / OPT_CHUNK; }
inline long long padded(long long numel) { return numel <= 0 ? 0 : (numel + 3) / 4 * 4; }

int plan_of(const int64_t* numels, int n_tensors, const char* who, ns_opt_plan* out) {
  const std::string w(who);
  if (!numels || !out) return api_fail(w + ": null argument");
  if (n_tensors <= 0) return api_fail(w + ": n_tensors must be positive, got " + std::to_string(n_tensors));
  long long chunks = 0, floats = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (numels[i] < 0) return api_fail(w + ": negative size of tensor " + std::to_string(i));
    if (numels[i] >= (1ll << 40)) return api_fail(w + ": problem too large");
    chunks += chunks_of(numels[i]);
    floats += padded(numels[i]);
    if (chunks >= (1ll << 31)) return api_fail(w + ": problem too large");
  }
  out->n_tensors = n_tensors;
  out->n_chunks = chunks;
  out->table_bytes = (int64_t)n_tensors * (int64_t)sizeof(ns_opt_tensor);
  out->ws_bytes = chunks * (int64_t)sizeof(double);
  out->state_floats = floats < 4 ? 4 : floats;
  return 0;
}

// what the four launching calls check
int opt_common(const ns_opt_plan* plan, const void* table, size_t table_bytes, const char* who) {
  const std::string w(who);
  if (!plan || !table) return api_fail(w + ": null argument");
  if (plan->n_tensors <= 0 || plan->n_tensors >= (1ll << 31)) return api_fail(w + ": n_tensors must be positive");
  if (plan->n_chunks < plan->n_tensors || plan->n_chunks >= (1ll << 31)) return api_fail(w + ": the plan's n_chunks is not one ns_opt_plan_sizes returns");
  if (plan->table_bytes != plan->n_tensors * (int64_t)sizeof(ns_opt_tensor) || plan->ws_bytes != plan->n_chunks * (int64_t)sizeof(double) || plan->state_floats < 4)
    return api_fail(w + ": the plan's sizes are not those ns_opt_plan_sizes returns");
  if (table_bytes < (size_t)plan->table_bytes) return api_fail(w + ": table too small (ns_opt_plan_sizes)");
  if ((uintptr_t)table & 7) return api_fail(w + ": table must be 8-byte aligned");
  return 0;
}
int record_ok(const ns_opt_record* r, const char* who) {
  if (!r) return api_fail(std::string(who) + ": null record");
  if ((uintptr_t)r & 7) return api_fail(std::string(who) + ": record must be 8-byte aligned");
  return 0;
}
}  // namespace

extern "C" int ns_opt_abi_version(void) { return NS_OPT_ABI_VERSION; }

extern "C" int ns_opt_plan_sizes(const int64_t* numels, int n_tensors, ns_opt_plan* out) { return plan_of(numels, n_tensors, "ns_opt_plan_sizes", out); }

extern "C" int ns_opt_build_table(const int64_t* numels, float* const* params, float* const* grads, const int32_t* lags, int n_tensors,
                                  void* table_host, size_t table_bytes) {
  const char* who = "ns_opt_build_table";
  ns_opt_plan plan;
  NS_TRY(plan_of(numels, n_tensors, who, &plan));
  if (!params || !grads || !table_host) return api_fail(std::string(who) + ": null argument");
  if (table_bytes < (size_t)plan.table_bytes) return api_fail(std::string(who) + ": table too small (ns_opt_plan_sizes)");
  if ((uintptr_t)table_host & 7) return api_fail(std::string(who) + ": table must be 8-byte aligned");
  for (int i = 0; i < n_tensors; ++i) {
    if (numels[i] > 0 && !params[i]) return api_fail(std::string(who) + ": null parameter pointer of tensor " + std::to_string(i));
    if (((uintptr_t)params[i] | (uintptr_t)grads[i]) & 3) return api_fail(std::string(who) + ": pointers of tensor " + std::to_string(i) + " must be 4-byte aligned");
    if (lags && lags[i] < 0) return api_fail(std::string(who) + ": negative lag of tensor " + std::to_string(i));
  }
  ns_opt_tensor* row = static_cast<ns_opt_tensor*>(table_host);
  long long chunk = 0, off = 0;
  for (int i = 0; i < n_tensors; ++i) {
    row[i].param = params[i];
    row[i].grad = numels[i] > 0 ? grads[i] : nullptr;  // an empty tensor has nothing to update: it is skipped
    row[i].numel = numels[i];
    row[i].state_offset = off;
    row[i].lag = lags ? lags[i] : 0;
    row[i].chunk_begin = (int32_t)chunk;
    chunk += chunks_of(numels[i]);
    off += padded(numels[i]);
  }
  return 0;
}

extern "C" int ns_opt_grad_norm(const ns_opt_plan* plan, const void* table, size_t table_bytes, float max_norm, void* ws, size_t ws_bytes,
                                ns_opt_record* record, void* stream) {
  const char* who = "ns_opt_grad_norm";
  NS_TRY(opt_common(plan, table, table_bytes, who));
  if (!ws) return api_fail(std::string(who) + ": null argument");
  NS_TRY(record_ok(record, who));
  if (ws_bytes < (size_t)plan->ws_bytes) return api_fail(std::string(who) + ": workspace too small (ns_opt_plan_sizes)");
  if ((uintptr_t)ws & 7) return api_fail(std::string(who) + ": workspace must be 8-byte aligned");
  if (!(max_norm >= 0.f)) return api_fail(std::string(who) + ": max_norm must be >= 0");
  NS_HIP(launch_opt_grad_norm(static_cast<const OptTensor*>(table), (int)plan->n_tensors, (int)plan->n_chunks, max_norm, static_cast<double*>(ws),
                              reinterpret_cast<OptRecord*>(record), (hipStream_t)stream));
  return 0;
}

extern "C" int ns_opt_scale_grads(const ns_opt_plan* plan, const void* table, size_t table_bytes, const ns_opt_record* record, void* stream) {
  const char* who = "ns_opt_scale_grads";
  NS_TRY(opt_common(plan, table, table_bytes, who));
  NS_TRY(record_ok(record, who));
  NS_HIP(launch_opt_scale(static_cast<const OptTensor*>(table), (int)plan->n_tensors, (int)plan->n_chunks, reinterpret_cast<const OptRecord*>(record),
                          (hipStream_t)stream));
  return 0;
}

extern "C" int ns_opt_adam_step(const ns_opt_plan* plan, const void* table, size_t table_bytes, const ns_opt_hyper* hyper, float* exp_avg,
                                float* exp_avg_sq, int64_t state_floats, const ns_opt_record* record, void* stream) {
  const char* who = "ns_opt_adam_step";
  const std::string w(who);
  NS_TRY(opt_common(plan, table, table_bytes, who));
  if (!hyper || !exp_avg || !exp_avg_sq) return api_fail(w + ": null argument");
  if (state_floats < 0) return api_fail(w + ": negative size");
  if (state_floats < plan->state_floats) return api_fail(w + ": state arena too small (ns_opt_plan_sizes)");
  if (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return api_fail(w + ": state arenas must be 16-byte aligned");
  if (exp_avg == exp_avg_sq) return api_fail(w + ": exp_avg and exp_avg_sq must be two arenas");
  if (!(hyper->beta1 >= 0.0 && hyper->beta1 < 1.0) || !(hyper->beta2 >= 0.0 && hyper->beta2 < 1.0)) return api_fail(w + ": betas must lie in [0, 1)");
  if (!(hyper->eps >= 0.0)) return api_fail(w + ": eps must be >= 0");
  if (!(hyper->lr >= 0.0)) return api_fail(w + ": lr must be >= 0");
  if (!(hyper->weight_decay >= 0.0)) return api_fail(w + ": weight_decay must be >= 0");
  if (hyper->global_step < 1) return api_fail(w + ": global_step must be >= 1, got " + std::to_string((long long)hyper->global_step));
  if (hyper->fuse_clip) NS_TRY(record_ok(record, who));
  OptHyper h;
  h.lr = hyper->lr; h.beta1 = hyper->beta1; h.beta2 = hyper->beta2; h.eps = hyper->eps; h.weight_decay = hyper->weight_decay;
  h.global_step = hyper->global_step; h.fuse_clip = hyper->fuse_clip != 0; h.zero_grads = hyper->zero_grads != 0;
  NS_HIP(launch_opt_adam(static_cast<const OptTensor*>(table), (int)plan->n_tensors, (int)plan->n_chunks, h, exp_avg, exp_avg_sq,
                         reinterpret_cast<const OptRecord*>(record), (hipStream_t)stream));
  return 0;
}

extern "C" int ns_opt_zero_grads(const ns_opt_plan* plan, const void* table, size_t table_bytes, void* stream) {
  NS_TRY(opt_common(plan, table, table_bytes, "ns_opt_zero_grads"));
  NS_HIP(launch_opt_zero(static_cast<const OptTensor*>(table), (int)plan->n_tensors, (int)plan->n_chunks, (hipStream_t)stream));
  return 0;
}
