// C-ABI of the wave-to-mel front end (include/nar_fs2.h ns_mel_*): the reference's TacotronSTFT.mel_spectrogram behind
// get_mel_from_wav's clip (audio/stft.py:52-81,159-178, audio/tools.py:8-15, audio/audio_processing.py:85-91) as three launches —
// hop rows (melfront.hip), the STFT as one fp32 Conv1D-as-GEMM (gemm_conv.hip launch_conv_gemm, called as it is), magnitude / energy /
// band-form mel (melfront.hip).  A separate handle with its own arena and workspace.  Host-side only; every byte of device memory
// comes from the caller.
#include <algorithm>
#include <cstdio>

#include "../../include/nar_fs2.h"
#include "host_core.h"

using namespace ns;

namespace {
const char* const K_FORWARD = "stft_fn.forward_basis";
const char* const K_INVERSE = "stft_fn.inverse_basis";  // the reference registers it too (stft.py:50); the forward never reads it
const char* const K_MEL = "mel_basis";
}  // namespace

struct ns_melfront {
  int fl, hop, win, n_mel, kw, bins;
  float clip;
  WeightRegistry weights;
  Arena ar;
  size_t w, band, bw;  // packed basis [fl][fl]; int {first bin, bins, offset} per filter; band weights (room for a dense matrix)
  float* arena = nullptr;
  bool ready = false;
  const float* P(size_t off) const { return arena + off; }
};

extern "C" int ns_mel_abi_version(void) { return NS_MEL_ABI_VERSION; }

extern "C" int64_t ns_mel_frames(int64_t n, int32_t hop) { return (n < 0 || hop < 1) ? 0 : n / hop + 1; }

extern "C" int ns_mel_create(const ns_mel_config* cfg, ns_melfront** out) {
  if (!cfg || !out) return api_fail("ns_mel_create: null argument");
  const ns_mel_config& c = *cfg;
  if (c.filter_length < 1 || c.hop_length < 1 || c.filter_length % c.hop_length)
    return api_fail("ns_mel_create: filter_length must be a positive multiple of hop_length (the STFT runs on rows of hop samples), got " +
                    std::to_string(c.filter_length) + " / " + std::to_string(c.hop_length));
  if (c.hop_length % 32) return api_fail("ns_mel_create: hop_length must be a multiple of 32 (the GEMM's K step), got " + std::to_string(c.hop_length));
  if (c.win_length < 1 || c.win_length > c.filter_length)
    return api_fail("ns_mel_create: win_length must be in [1, filter_length] (stft.py:39), got " + std::to_string(c.win_length));
  if (c.n_mel < 4 || c.n_mel % 4) return api_fail("ns_mel_create: n_mel must be a positive multiple of 4, got " + std::to_string(c.n_mel));
  if (!(c.clip_val > 0.f)) return api_fail("ns_mel_create: clip_val must be positive (log of the clamp, audio_processing.py:91)");
  // N = KW * Cin = filter_length: the dispatch's own verdict on the shape, plus the magnitude row k_mel_project stages in LDS
  int rec[2][8];
  if (c.filter_length > MEL_MAX_FILTER || conv_gemm_describe(1024, c.filter_length, c.hop_length, c.filter_length / c.hop_length, 0, rec) == 0)
    return api_fail("ns_mel_create: filter_length " + std::to_string(c.filter_length) + " is outside the range of the STFT GEMM (N = KW * Cin = filter_length <= " +
                    std::to_string(MEL_MAX_FILTER) + ")");
  ns_melfront* h = new ns_melfront();
  h->fl = c.filter_length; h->hop = c.hop_length; h->win = c.win_length; h->n_mel = c.n_mel; h->clip = c.clip_val;
  h->kw = h->fl / h->hop; h->bins = h->fl / 2 + 1;
  h->weights.expect(K_FORWARD, {h->fl + 2, 1, h->fl});
  h->weights.expect(K_MEL, {h->n_mel, h->bins});
  h->w = h->ar.take((size_t)h->fl * h->fl);
  h->band = h->ar.take((size_t)3 * h->n_mel);
  h->bw = h->ar.take((size_t)h->n_mel * h->bins);
  *out = h;
  return 0;
}

extern "C" void ns_mel_destroy(ns_melfront* h) { delete h; }
extern "C" size_t ns_mel_arena_bytes(const ns_melfront* h) { return h ? h->ar.n * sizeof(float) : 0; }

extern "C" int ns_mel_bind_arena(ns_melfront* h, void* dev, size_t bytes) {
  return bind_arena(h, dev, bytes, ns_mel_arena_bytes(h), "ns_mel_bind_arena", "arena too small (ns_mel_arena_bytes)");
}

extern "C" int ns_mel_check_weight(ns_melfront* h, const char* name, const int64_t* shape, int ndim) {
  if (h && name && !strcmp(name, K_INVERSE)) return 0;
  return check_weight(h, name, shape, ndim, "ns_mel_check_weight");
}

extern "C" int ns_mel_set_weight(ns_melfront* h, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (h && name && !strcmp(name, K_INVERSE)) return 0;
  return set_weight(h, name, host, shape, ndim, "ns_mel_set_weight");
}

extern "C" int ns_mel_finalize_weights(ns_melfront* h, void* stream) {
  if (!h) return api_fail("ns_mel_finalize_weights: null argument");
  if (!h->arena) return api_fail("ns_mel_finalize_weights: no arena bound (ns_mel_bind_arena)");
  const std::vector<std::string> missing = h->weights.missing();
  if (!missing.empty()) return api_fail("ns_mel_finalize_weights: missing keys: " + join_names(missing));
  const std::vector<float>& fb = h->weights.data(K_FORWARD);
  const std::vector<float>& mb = h->weights.data(K_MEL);
  const int fl = h->fl, bins = h->bins, half = fl / 2;
  // rows 0 .. bins-1 are the real parts, bins .. 2 bins - 1 the imaginary ones (stft.py:29-31); sin(0) and sin(pi n) rows are zero
  for (int k : {0, half})
    for (int n = 0; n < fl; ++n)
      if (!(std::fabs(fb[(size_t)(bins + k) * fl + n]) <= 1e-6f))
        return api_fail("ns_mel_finalize_weights: stft_fn.forward_basis is not a real DFT basis: the imaginary row of bin " + std::to_string(k) +
                        " holds an entry of magnitude above 1e-6");
  std::vector<float> img(h->ar.n, 0.f);
  // packed real DFT: GEMM column 0 = re_0, 1 = re_{fl/2}, 2k = re_k, 2k + 1 = im_k; a weight row IS the basis row, because the packed
  // K index j * hop + c is the sample index inside the frame
  auto row = [&](int dst, int src) { std::copy(fb.begin() + (size_t)src * fl, fb.begin() + (size_t)(src + 1) * fl, img.begin() + h->w + (size_t)dst * fl); };
  row(0, 0);
  row(1, half);
  for (int k = 1; k < half; ++k) { row(2 * k, k); row(2 * k + 1, bins + k); }
  // band form: first to last non-zero bin of every filter, interior zeros kept
  int32_t* band = reinterpret_cast<int32_t*>(&img[h->band]);
  size_t used = 0;
  for (int m = 0; m < h->n_mel; ++m) {
    int lo = bins, hi = -1;
    for (int k = 0; k < bins; ++k)
      if (mb[(size_t)m * bins + k] != 0.f) { lo = std::min(lo, k); hi = k; }
    const int nk = hi >= lo ? hi - lo + 1 : 0;
    band[3 * m] = nk ? lo : 0; band[3 * m + 1] = nk; band[3 * m + 2] = (int32_t)used;
    for (int i = 0; i < nk; ++i) img[h->bw + used + i] = mb[(size_t)m * bins + lo + i];
    used += nk;
  }
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(hipMemcpyAsync(h->arena, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st));
  NS_HIP(hipStreamSynchronize(st));  // img is a local
  h->weights.release();
  h->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ workspace
// frames actually computed for a caller's T: no utterance has more than ns_mel_frames(n_max) of them, the rest are zero-filled
static int computed_frames(const ns_melfront* h, int64_t n_max, int T) {
  const int64_t f = ns_mel_frames(n_max, h->hop);
  return (int)std::min<int64_t>(T, f);
}

extern "C" size_t ns_mel_ws_bytes(const ns_melfront* h, int B, int64_t n_max) {
  if (!h || B <= 0 || n_max < 0) return 256;
  const size_t S = (size_t)ns_mel_frames(n_max, h->hop) + h->kw - 1;
  Bump bp(nullptr);
  bp.f((size_t)B * S * h->hop);
  bp.f((size_t)B * S * h->fl);
  return bp.off + 256;
}

static int check_ready(const ns_melfront* h, const char* who) {
  if (!h) return api_fail(std::string(who) + ": null handle");
  if (!h->ready || !h->arena) return api_fail(std::string(who) + ": weights not finalized (ns_mel_finalize_weights)");
  return 0;
}

static int stft(const ns_melfront* h, const float* rows, int B, int S, float* spec, hipStream_t st) {
  ConvGemm p;
  memset(&p, 0, sizeof(p));
  p.X = rows; p.ldx = h->hop; p.W = h->P(h->w); p.Y = spec; p.ldy = h->fl;
  p.M = B * S; p.N = h->fl; p.Cin = h->hop; p.KW = h->kw; p.pad = 0; p.S = S; p.act = ACT_NONE; p.epi = EPI_NONE;
  NS_HIP(launch_conv_gemm(p, st));
  return 0;
}

static int check_sizes(const ns_melfront* h, int B, int S, const char* who) {
  if ((long long)B * S >= (1ll << 31) / h->fl) return api_fail(std::string(who) + ": problem too large (B * rows * filter_length must stay below 2^31: split the batch)");
  if (B > 65535) return api_fail(std::string(who) + ": B must be at most 65535");
  return 0;
}

extern "C" int ns_mel_forward(ns_melfront* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int T, float* mel,
                              float* energy, int64_t* mel_lens_out, void* ws, size_t ws_bytes, void* stream) {
  NS_TRY(check_ready(h, "ns_mel_forward"));
  if (B < 0 || n_max < 0) return api_fail("ns_mel_forward: negative size");
  if (T < 1) return api_fail("ns_mel_forward: T must be >= 1");
  if (B == 0) return 0;
  if (!wav || !wav_lens || !mel || !energy || !mel_lens_out || !ws) return api_fail("ns_mel_forward: null argument");
  if (ld_wav < n_max) return api_fail("ns_mel_forward: ld_wav must be >= n_max");
  if (ws_bytes < ns_mel_ws_bytes(h, B, n_max)) return api_fail("ns_mel_forward: workspace too small (ns_mel_ws_bytes)");
  if ((uintptr_t)ws & 255) return api_fail("ns_mel_forward: workspace must be 256-byte aligned");
  if ((long long)B * T >= (1ll << 31) / h->n_mel) return api_fail("ns_mel_forward: problem too large (B * T * n_mel must stay below 2^31)");
  const int Tc = computed_frames(h, n_max, T), S = Tc + h->kw - 1;
  NS_TRY(check_sizes(h, B, S, "ns_mel_forward"));
  hipStream_t st = (hipStream_t)stream;
  const long long* lens = reinterpret_cast<const long long*>(wav_lens);
  Bump bp(ws);
  float* rows = bp.f((size_t)B * S * h->hop);
  float* spec = bp.f((size_t)B * S * h->fl);
  NS_HIP(launch_mel_frame_rows(wav, ld_wav, lens, B, n_max, h->fl, h->hop, S, rows, reinterpret_cast<long long*>(mel_lens_out), st));
  NS_TRY(stft(h, rows, B, S, spec, st));
  NS_HIP(launch_mel_project(spec, lens, B, S, n_max, T, h->fl, h->hop, h->n_mel, h->clip, reinterpret_cast<const int*>(h->P(h->band)), h->P(h->bw),
                            mel, energy, st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ per-operator entry points
extern "C" int ns_mel_op_frame_rows(ns_melfront* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int S,
                                    float* rows, int64_t* mel_lens_out, void* stream) {
  if (!h || !wav || !wav_lens || !rows || B <= 0 || S < 1 || n_max < 0 || ld_wav < n_max) return api_fail("ns_mel_op_frame_rows: bad argument");
  if ((uintptr_t)rows & 15) return api_fail("ns_mel_op_frame_rows: rows must be 16-byte aligned");
  NS_TRY(check_sizes(h, B, S, "ns_mel_op_frame_rows"));
  NS_HIP(launch_mel_frame_rows(wav, ld_wav, reinterpret_cast<const long long*>(wav_lens), B, n_max, h->fl, h->hop, S, rows,
                               reinterpret_cast<long long*>(mel_lens_out), (hipStream_t)stream));
  return 0;
}

extern "C" int ns_mel_op_stft(ns_melfront* h, const float* rows, int B, int S, float* spec, void* stream) {
  NS_TRY(check_ready(h, "ns_mel_op_stft"));
  if (!rows || !spec || B <= 0 || S < 1) return api_fail("ns_mel_op_stft: bad argument");
  if (((uintptr_t)rows | (uintptr_t)spec) & 15) return api_fail("ns_mel_op_stft: rows and spec must be 16-byte aligned");
  NS_TRY(check_sizes(h, B, S, "ns_mel_op_stft"));
  return stft(h, rows, B, S, spec, (hipStream_t)stream);
}

extern "C" int ns_mel_op_project(ns_melfront* h, const float* spec, const int64_t* wav_lens, int B, int S, int64_t n_max, int T, float* mel,
                                 float* energy, void* stream) {
  NS_TRY(check_ready(h, "ns_mel_op_project"));
  if (!spec || !wav_lens || !mel || !energy || B <= 0 || S < h->kw || T < 1 || n_max < 0) return api_fail("ns_mel_op_project: bad argument");
  if ((uintptr_t)spec & 15) return api_fail("ns_mel_op_project: spec must be 16-byte aligned");
  NS_TRY(check_sizes(h, B, S, "ns_mel_op_project"));
  if ((long long)B * T >= (1ll << 31) / h->n_mel) return api_fail("ns_mel_op_project: problem too large");
  NS_HIP(launch_mel_project(spec, reinterpret_cast<const long long*>(wav_lens), B, S, n_max, T, h->fl, h->hop, h->n_mel, h->clip,
                            reinterpret_cast<const int*>(h->P(h->band)), h->P(h->bw), mel, energy, (hipStream_t)stream));
  return 0;
}
