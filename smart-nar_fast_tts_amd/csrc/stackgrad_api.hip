// C-ABI of the pieces the TxtEncoder and MelDecoder training stacks add to their FFT blocks (include/nar_fs2.h ns_st_*;
// transformer/Models.py:33-100, 176-244).  No handle and no workspace: every tensor is the caller's.  Host-side
// only; every argument is validated before the first HIP call.  The two forward ops launch rowops.hip's kernels as they are
// (k_embed_pos with nothing to zero, k_add_pos on dense rows); the table gradient and the row mask are stackgrad.hip's.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

namespace {
thread_local int t_launches = 0;

// what the four ops check alike: B, S and D of [B, S, D] rows (the table gradient passes its M rows as B = M, S = 1)
int check_rows(const std::string& w, int B, int S, int D) {
  if (B <= 0 || S <= 0) return api_fail(w + "B and S must be positive, got " + std::to_string(B) + " x " + std::to_string(S));
  if (D != 256 && D != 512) return api_fail(w + "D must be 256 or 512, got " + std::to_string(D));
  if ((long long)B * S * D >= (1ll << 31)) return api_fail(w + "problem too large: B * S * D must stay below 2^31");
  return 0;
}

int check_vocab(const std::string& w, int n_vocab) {
  if (n_vocab < 2) return api_fail(w + "n_vocab must be at least 2 (PAD and one symbol), got " + std::to_string(n_vocab));
  return 0;
}
}  // namespace

extern "C" int ns_st_abi_version(void) { return NS_ST_ABI_VERSION; }
extern "C" int ns_st_last_launches(void) { return t_launches; }

extern "C" int ns_st_op_embed_pos(const int64_t* texts, const float* emb, const float* pos, int B, int S, int D, int n_vocab, float* out,
                                  void* stream) {
  const std::string w = "ns_st_op_embed_pos: ";
  t_launches = 0;
  if (!texts || !emb || !pos || !out) return api_fail(w + "null argument");
  NS_TRY(check_rows(w, B, S, D));
  NS_TRY(check_vocab(w, n_vocab));
  NS_TRY(check_aligned(w, {{"emb", emb}, {"pos", pos}, {"out", out}, {"texts", texts, 8}}));
  NS_HIP(launch_embed_pos((const long long*)texts, emb, pos, out, B * S, S, D, n_vocab, nullptr, 0, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_st_op_add_pos(const float* x, const float* pos, int B, int S, int D, float* out, void* stream) {
  const std::string w = "ns_st_op_add_pos: ";
  t_launches = 0;
  if (!x || !pos || !out) return api_fail(w + "null argument");
  NS_TRY(check_rows(w, B, S, D));
  NS_TRY(check_aligned(w, {{"x", x}, {"pos", pos}, {"out", out}}));
  NS_HIP(launch_add_pos(x, pos, out, B * S, S, D, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_st_op_embed_grad(const float* g, const int64_t* texts, int M, int D, int n_vocab, float* d_table, void* stream) {
  const std::string w = "ns_st_op_embed_grad: ";
  t_launches = 0;
  if (!g || !texts || !d_table) return api_fail(w + "null argument");
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  NS_TRY(check_rows(w, M, 1, D));
  NS_TRY(check_vocab(w, n_vocab));
  NS_TRY(check_aligned(w, {{"g", g}, {"d_table", d_table}, {"texts", texts, 8}}));
  NS_HIP(launch_st_embed_grad(g, (const long long*)texts, M, D, n_vocab, d_table, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_st_op_row_mask(const float* x, const uint8_t* mask, const int64_t* lens, int B, int S, int D, float* y, void* stream) {
  const std::string w = "ns_st_op_row_mask: ";
  t_launches = 0;
  if (!x || !y) return api_fail(w + "null argument");
  if (!mask && !lens) return api_fail(w + "neither mask nor lens given");
  NS_TRY(check_rows(w, B, S, D));
  if (x == y) return api_fail(w + "y must not be x (the op is out of place)");
  NS_TRY(check_aligned(w, {{"x", x}, {"y", y}, {"lens", lens, 8}}));
  NS_HIP(launch_st_row_mask(x, mask, (const long long*)lens, B * S, S, D, y, (hipStream_t)stream));
  ++t_launches;
  return 0;
}
