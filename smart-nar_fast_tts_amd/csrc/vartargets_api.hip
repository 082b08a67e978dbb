// C-ABI of the variance targets and dataset statistics (include/nar_fs2.h ns_vt_*): the tail of the reference's
// Preprocessor.process_utterance and its build_from_path / remove_outlier / normalize (preprocessor/preprocessor.py:188-227, 61-133,
// 289-310).  No handle: there are no weights.  Host-side only; every byte of device memory comes from the caller, and every argument
// is validated before the first HIP call.
#include "../../include/nar_fs2.h"
#include "host_core.h"

using namespace ns;

static_assert(sizeof(ns_vt_state) == sizeof(VtState) && sizeof(ns_vt_state) == 80, "ns_vt_state layout");
static_assert(NS_VT_SORT_CAPACITY == VT_SORT_CAPACITY, "sort capacity");

namespace {
// what all three calls check; `who` names the entry point
int vt_common(const ns_vt_args* a, const void* ws, size_t ws_bytes, const char* who, VtArgs* k) {
  const std::string w(who);
  if (!a || !ws) return api_fail(w + ": null argument");
  if (a->B < 0 || a->L < 0 || a->T < 0) return api_fail(w + ": negative size");
  const long long frames = (long long)a->B * a->T, phonemes = (long long)a->B * a->L;
  if (frames >= (1ll << 31) || phonemes >= (1ll << 31) || a->L >= (1 << 26)) return api_fail(w + ": problem too large");
  if (a->B > 0 && !a->src_lens) return api_fail(w + ": null src_lens");
  if (a->B > 0 && !a->frame_lens) return api_fail(w + ": null frame_lens");
  if ((a->pitch_frame_level ? frames : phonemes) > 0 && !a->pitch_targets) return api_fail(w + ": null pitch_targets");
  if ((a->energy_frame_level ? frames : phonemes) > 0 && !a->energy_targets) return api_fail(w + ": null energy_targets");
  if (ws_bytes < ns_vt_ws_bytes(a->B, a->L, a->T)) return api_fail(w + ": workspace too small (ns_vt_ws_bytes)");
  if ((uintptr_t)ws & 15) return api_fail(w + ": workspace must be 16-byte aligned");
  k->B = a->B; k->L = a->L; k->T = a->T;
  k->pitch_frame_level = a->pitch_frame_level != 0; k->energy_frame_level = a->energy_frame_level != 0;
  k->pitch_normalization = a->pitch_normalization != 0; k->energy_normalization = a->energy_normalization != 0;
  k->durations_stride = a->durations_stride;
  k->pitch = a->pitch; k->energy = a->energy;
  k->durations = reinterpret_cast<const long long*>(a->durations); k->src_lens = reinterpret_cast<const long long*>(a->src_lens);
  k->pitch_targets = a->pitch_targets; k->energy_targets = a->energy_targets;
  k->frame_lens = reinterpret_cast<long long*>(a->frame_lens); k->valid = a->valid;
  return 0;
}
int vt_state_ok(const ns_vt_state* s, const char* who) {
  if (!s) return api_fail(std::string(who) + ": null state");
  if ((uintptr_t)s & 7) return api_fail(std::string(who) + ": state must be 8-byte aligned");
  return 0;
}
}  // namespace

extern "C" int ns_vt_abi_version(void) { return NS_VT_ABI_VERSION; }

extern "C" size_t ns_vt_ws_bytes(int B, int L, int T) { return vt_ws_bytes(B, L, T); }

extern "C" int ns_vt_state_init(ns_vt_state* state, void* stream) {
  NS_TRY(vt_state_ok(state, "ns_vt_state_init"));
  NS_HIP(launch_vt_state_init(reinterpret_cast<VtState*>(state), (hipStream_t)stream));
  return 0;
}

extern "C" int ns_vt_targets(const ns_vt_args* a, void* ws, size_t ws_bytes, void* stream) {
  VtArgs k;
  NS_TRY(vt_common(a, ws, ws_bytes, "ns_vt_targets", &k));
  if (a->B > 0 && !a->valid) return api_fail("ns_vt_targets: null valid");
  if ((long long)a->B * a->T > 0 && (!a->pitch || !a->energy)) return api_fail("ns_vt_targets: null pitch or energy");
  if ((long long)a->B * a->L > 0) {
    if (!a->durations) return api_fail("ns_vt_targets: null durations");
    if (a->durations_stride < a->L) return api_fail("ns_vt_targets: durations_stride must be at least L, got " + std::to_string(a->durations_stride));
  }
  NS_HIP(launch_vt_targets(k, ws, (hipStream_t)stream));
  return 0;
}

extern "C" int ns_vt_fit(const ns_vt_args* a, ns_vt_state* state, void* ws, size_t ws_bytes, void* stream) {
  VtArgs k;
  NS_TRY(vt_common(a, ws, ws_bytes, "ns_vt_fit", &k));
  NS_TRY(vt_state_ok(state, "ns_vt_fit"));
  if (a->B > 0 && !a->valid) return api_fail("ns_vt_fit: null valid");
  const int n_pitch = a->pitch_frame_level ? a->T : a->L, n_energy = a->energy_frame_level ? a->T : a->L;
  if (n_pitch > NS_VT_SORT_CAPACITY || n_energy > NS_VT_SORT_CAPACITY)
    return api_fail("ns_vt_fit: " + std::to_string(n_pitch > n_energy ? n_pitch : n_energy) + " values per utterance exceed the LDS sort capacity NS_VT_SORT_CAPACITY = " +
                    std::to_string(NS_VT_SORT_CAPACITY));
  NS_HIP(launch_vt_fit(k, reinterpret_cast<VtState*>(state), ws, (hipStream_t)stream));
  return 0;
}

extern "C" int ns_vt_normalize(const ns_vt_args* a, ns_vt_state* state, void* ws, size_t ws_bytes, void* stream) {
  VtArgs k;
  NS_TRY(vt_common(a, ws, ws_bytes, "ns_vt_normalize", &k));
  NS_TRY(vt_state_ok(state, "ns_vt_normalize"));
  NS_HIP(launch_vt_normalize(k, reinterpret_cast<VtState*>(state), ws, (hipStream_t)stream));
  return 0;
}
