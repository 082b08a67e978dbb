// C-ABI of the validation loss (include/nar_fs2.h ns_loss_*): the reference's FastSpeech2Loss.forward (model/loss.py:149-250) on one
// teacher-forced batch.  No handle: the loss has no weights.  Host-side only; every byte of device memory comes from the caller,
// and every argument is validated before the first HIP call.
#include "loss_check.h"

using namespace ns;

extern "C" int ns_loss_abi_version(void) { return NS_LOSS_ABI_VERSION; }

extern "C" size_t ns_loss_ws_bytes(int B, int L, int T) {
  if (B <= 0 || L < 0 || T < 0) return LOSS_SLOT_BYTES;
  return (size_t)(loss_slots(B, L, T, nullptr, nullptr) + 1) * LOSS_SLOT_BYTES;
}

// What ns_loss_forward and the ns_lossg_* calls (lossgrad_api.hip) check of the argument block, in this order; fills the kernels' mirror.
int ns::loss_check_args(const ns_loss_args* a, const char* who, LossArgs* out) {
  const std::string w = std::string(who) + ": ";
  if (a->B < 0 || a->L < 0 || a->T < 0) return api_fail(w + "negative size");
  if (a->n_mel <= 0 || (a->n_mel & 3)) return api_fail(w + "n_mel must be a positive multiple of 4 (rows are read as float4), got " + std::to_string(a->n_mel));
  const long long frames = (long long)a->B * a->T, phonemes = (long long)a->B * a->L;
  if (frames >= (1ll << 31) || phonemes >= (1ll << 31) || a->L >= (1 << 26)) return api_fail(w + "problem too large");
  const bool cells = frames > 0 && a->L > 0;
  if (cells && a->H < 1) return api_fail(w + "H must be >= 1 (head 0 of every map is read, model/loss.py:233-236)");
  if (a->B > 0 && (!a->src_lens || !a->mel_lens)) return api_fail(w + "null src_lens or mel_lens");
  if (frames > 0) {
    if (!a->mel || !a->postnet || !a->mel_targets || !a->mel_masks) return api_fail(w + "null mel, postnet, mel_targets or mel_masks");
    if (a->mel_targets_stride < (long long)a->T * a->n_mel || (a->mel_targets_stride & 3))
      return api_fail(w + "mel_targets_stride must be a multiple of 4 and at least T * n_mel (mel_targets[:, :T], model/loss.py:191)");
    if (((uintptr_t)a->mel | (uintptr_t)a->postnet | (uintptr_t)a->mel_targets) & 15) return api_fail(w + "mel, postnet and mel_targets must be 16-byte aligned");
  }
  if (phonemes > 0) {
    if (!a->log_d || !a->d_targets || !a->src_masks) return api_fail(w + "null log_d, d_targets or src_masks");
    if (a->d_targets_stride < a->L) return api_fail(w + "d_targets_stride must be at least L (duration_targets[:, :L], model/loss.py:214-216)");
  }
  if ((a->pitch_frame_level ? frames : phonemes) > 0 && (!a->pitch || !a->pitch_targets)) return api_fail(w + "null pitch or pitch_targets");
  if ((a->energy_frame_level ? frames : phonemes) > 0 && (!a->energy || !a->energy_targets)) return api_fail(w + "null energy or energy_targets");
  if (cells)
    for (int k = 0; k < 4; ++k)
      if (!a->attn[k] || ((uintptr_t)a->attn[k] & 3)) return api_fail(w + "attn[" + std::to_string(k) + "] is null or not 4-byte aligned (four maps are read, model/loss.py:233-236)");
  LossArgs& k = *out;
  k.B = a->B; k.L = a->L; k.T = a->T; k.H = a->H; k.n_mel = a->n_mel;
  k.pitch_frame_level = a->pitch_frame_level != 0; k.energy_frame_level = a->energy_frame_level != 0;
  k.mel_targets_stride = a->mel_targets_stride; k.d_targets_stride = a->d_targets_stride;
  k.mel = a->mel; k.postnet = a->postnet; k.mel_targets = a->mel_targets; k.mel_masks = a->mel_masks;
  k.pitch = a->pitch; k.pitch_targets = a->pitch_targets; k.energy = a->energy; k.energy_targets = a->energy_targets;
  k.log_d = a->log_d; k.d_targets = reinterpret_cast<const long long*>(a->d_targets); k.src_masks = a->src_masks;
  k.src_lens = reinterpret_cast<const long long*>(a->src_lens); k.mel_lens = reinterpret_cast<const long long*>(a->mel_lens);
  for (int i = 0; i < 4; ++i) k.attn[i] = a->attn[i];
  return 0;
}

int ns::loss_check_ws(const ns_loss_args* a, const void* ws, size_t ws_bytes, const float* out7, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (ws_bytes < ns_loss_ws_bytes(a->B, a->L, a->T)) return api_fail(w + "workspace too small (ns_loss_ws_bytes)");
  if (((uintptr_t)ws & 15) || ((uintptr_t)out7 & 3)) return api_fail(w + "workspace must be 16-byte aligned, out7 4-byte aligned");
  return 0;
}

extern "C" int ns_loss_forward(const ns_loss_args* a, void* ws, size_t ws_bytes, float* out7, void* stream) {
  if (!a || !ws || !out7) return api_fail("ns_loss_forward: null argument");
  LossArgs k;
  NS_TRY(loss_check_args(a, "ns_loss_forward", &k));
  NS_TRY(loss_check_ws(a, ws, ws_bytes, out7, "ns_loss_forward"));
  NS_HIP(launch_loss(k, ws, out7, (hipStream_t)stream));
  return 0;
}
