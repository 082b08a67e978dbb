// C-ABI of the training loss (include/nar_fs2.h ns_lossg_*): FastSpeech2Loss's value with the record of its counts, and its backward
// (train.py:83-88 through model/loss.py:149-250).  No handle; the argument block is ns_loss_args and is checked by the same code as
// ns_loss_forward (loss_check.h).  Host-side only; every argument is validated before the first HIP call.
#include "loss_check.h"

using namespace ns;

static_assert(NS_LOSSG_RECORD_BYTES == LOSSG_RECORD_BYTES && LOSSG_RECORD_BYTES == 8 * LOSSG_RECORD_WORDS, "record layout");
static_assert(sizeof(ns_lossg_grads) == sizeof(LossGrads) && sizeof(ns_lossg_grads) == 9 * sizeof(void*), "ns_lossg_grads layout");

extern "C" int ns_lossg_abi_version(void) { return NS_LOSSG_ABI_VERSION; }

extern "C" size_t ns_lossg_record_bytes(void) { return NS_LOSSG_RECORD_BYTES; }

extern "C" int ns_lossg_forward(const ns_loss_args* a, void* ws, size_t ws_bytes, float* out7, void* record, void* stream) {
  const char* who = "ns_lossg_forward";
  if (!a || !ws || !out7 || !record) return api_fail(std::string(who) + ": null argument");
  LossArgs k;
  NS_TRY(loss_check_args(a, who, &k));
  NS_TRY(loss_check_ws(a, ws, ws_bytes, out7, who));
  if ((uintptr_t)record & 7) return api_fail(std::string(who) + ": record must be 8-byte aligned");
  NS_HIP(launch_loss(k, ws, out7, (hipStream_t)stream, reinterpret_cast<long long*>(record)));
  return 0;
}

extern "C" int ns_lossg_backward(const ns_loss_args* a, const void* record, const float* g7, const ns_lossg_grads* grads, void* stream) {
  const std::string w = "ns_lossg_backward: ";
  if (!a || !record || !g7 || !grads) return api_fail(w + "null argument");
  LossArgs k;
  NS_TRY(loss_check_args(a, "ns_lossg_backward", &k));
  if ((long long)a->B * a->H * a->T >= (1ll << 31)) return api_fail(w + "problem too large");
  if (((uintptr_t)record & 7) || ((uintptr_t)g7 & 3)) return api_fail(w + "record must be 8-byte aligned, g7 4-byte aligned");
  LossGrads d;
  d.mel = grads->mel; d.postnet = grads->postnet; d.pitch = grads->pitch; d.energy = grads->energy; d.log_d = grads->log_d;
  for (int i = 0; i < 4; ++i) d.attn[i] = grads->attn[i];
  const void* outs[9] = {d.mel, d.postnet, d.pitch, d.energy, d.log_d, d.attn[0], d.attn[1], d.attn[2], d.attn[3]};
  const char* names[9] = {"mel", "postnet", "pitch", "energy", "log_d", "attn[0]", "attn[1]", "attn[2]", "attn[3]"};
  for (int i = 0; i < 9; ++i)
    if ((uintptr_t)outs[i] & 15) return api_fail(w + "grads->" + names[i] + " must be 16-byte aligned (gradients are stored as 16-byte vectors)");
  NS_HIP(launch_lossg(k, reinterpret_cast<const long long*>(record), g7, d, (hipStream_t)stream));
  return 0;
}
