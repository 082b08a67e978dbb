// C-ABI of the Griffin-Lim mel-to-wave path (include/nar_fs2.h ns_gl_*): the reference's inv_mel_spec (audio/tools.py:18-34),
// griffin_lim (audio/audio_processing.py:66-82), STFT.inverse and STFT.transform (audio/stft.py:52-122).  One iteration is two fp32
// Conv1D-as-GEMM calls (gemm_conv.hip launch_conv_gemm, called as it is) and three row-local launches (griffinlim.hip, melfront.hip's
// non-clipping hop rows).  A separate handle with its own arena and workspace.  Host-side only; every byte of device memory comes from
// the caller, and nothing here reads the device.
#include <algorithm>

#include "../../include/nar_fs2.h"
#include "host_core.h"

using namespace ns;

namespace {
const char* const K_FORWARD = "stft_fn.forward_basis";
const char* const K_INVERSE = "stft_fn.inverse_basis";
const char* const K_MEL = "mel_basis";
const double PI = 3.14159265358979323846;
}  // namespace

struct ns_gl {
  int fl, hop, win, n_mel, kw, bins;
  float scaling;
  WeightRegistry weights;
  Arena ar;
  size_t wf, wi, mb, wsq;  // packed forward basis [fl][fl]; inverse weight [fl samples][fl packed columns]; mel_basis; fl doubles
  float* arena = nullptr;
  bool ready = false, has_mel = false;
  const float* P(size_t off) const { return arena + off; }
};

extern "C" int ns_gl_abi_version(void) { return NS_GL_ABI_VERSION; }

extern "C" int ns_gl_create(const ns_gl_config* cfg, ns_gl** out) {
  if (!cfg || !out) return api_fail("ns_gl_create: null argument");
  const ns_gl_config& c = *cfg;
  if (c.filter_length < 1 || c.hop_length < 1 || c.filter_length % c.hop_length)
    return api_fail("ns_gl_create: filter_length must be a positive multiple of hop_length (the STFT runs on rows of hop samples), got " +
                    std::to_string(c.filter_length) + " / " + std::to_string(c.hop_length));
  if (c.hop_length % 32) return api_fail("ns_gl_create: hop_length must be a multiple of 32 (the GEMM's K step), got " + std::to_string(c.hop_length));
  if (c.win_length < 1 || c.win_length > c.filter_length)
    return api_fail("ns_gl_create: win_length must be in [1, filter_length] (stft.py:39), got " + std::to_string(c.win_length));
  if (c.n_mel < 4 || c.n_mel % 4) return api_fail("ns_gl_create: n_mel must be a positive multiple of 4, got " + std::to_string(c.n_mel));
  if (!(c.spec_from_mel_scaling > 0.f)) return api_fail("ns_gl_create: spec_from_mel_scaling must be positive (tools.py:22)");
  int rec[2][8];
  if (c.filter_length > MEL_MAX_FILTER || conv_gemm_describe(1024, c.filter_length, c.hop_length, c.filter_length / c.hop_length, 0, rec) == 0 ||
      conv_gemm_describe(1024, c.filter_length, c.filter_length, 1, 0, rec) == 0)
    return api_fail("ns_gl_create: filter_length " + std::to_string(c.filter_length) + " is outside the range of the STFT GEMMs (N = K = filter_length <= " +
                    std::to_string(MEL_MAX_FILTER) + ")");
  ns_gl* h = new ns_gl();
  h->fl = c.filter_length; h->hop = c.hop_length; h->win = c.win_length; h->n_mel = c.n_mel; h->scaling = c.spec_from_mel_scaling;
  h->kw = h->fl / h->hop; h->bins = h->fl / 2 + 1;
  h->weights.expect(K_FORWARD, {h->fl + 2, 1, h->fl});
  h->weights.expect(K_INVERSE, {h->fl + 2, 1, h->fl});
  h->weights.expect(K_MEL, {h->n_mel, h->bins}, /*optional=*/true);  // a bare STFT (audio.STFT) has none: the mel entry points then refuse
  h->wf = h->ar.take((size_t)h->fl * h->fl);
  h->wi = h->ar.take((size_t)h->fl * h->fl);
  h->mb = h->ar.take((size_t)h->n_mel * h->bins);
  h->wsq = h->ar.take((size_t)2 * h->fl);
  *out = h;
  return 0;
}

extern "C" void ns_gl_destroy(ns_gl* h) { delete h; }
extern "C" size_t ns_gl_arena_bytes(const ns_gl* h) { return h ? h->ar.n * sizeof(float) : 0; }

extern "C" int ns_gl_bind_arena(ns_gl* h, void* dev, size_t bytes) {
  return bind_arena(h, dev, bytes, ns_gl_arena_bytes(h), "ns_gl_bind_arena", "arena too small (ns_gl_arena_bytes)");
}

extern "C" int ns_gl_check_weight(ns_gl* h, const char* name, const int64_t* shape, int ndim) {
  return check_weight(h, name, shape, ndim, "ns_gl_check_weight");
}

extern "C" int ns_gl_set_weight(ns_gl* h, const char* name, const float* host, const int64_t* shape, int ndim) {
  return set_weight(h, name, host, shape, ndim, "ns_gl_set_weight");
}

extern "C" int ns_gl_finalize_weights(ns_gl* h, void* stream) {
  if (!h) return api_fail("ns_gl_finalize_weights: null argument");
  if (!h->arena) return api_fail("ns_gl_finalize_weights: no arena bound (ns_gl_bind_arena)");
  const std::vector<std::string> missing = h->weights.missing();
  if (!missing.empty()) return api_fail("ns_gl_finalize_weights: missing keys: " + join_names(missing));
  const std::vector<float>& fb = h->weights.data(K_FORWARD);
  const std::vector<float>& ib = h->weights.data(K_INVERSE);
  const int fl = h->fl, bins = h->bins, half = fl / 2;
  // rows 0 .. bins-1 are the real parts, bins .. 2 bins - 1 the imaginary ones (stft.py:29-36).  The packed layout drops the
  // imaginary rows of bins 0 and fl / 2: zero in a real DFT basis, and zero in its pseudo-inverse (stft.py:35)
  for (int k : {0, half})
    for (int n = 0; n < fl; ++n) {
      if (!(std::fabs(fb[(size_t)(bins + k) * fl + n]) <= 1e-6f))
        return api_fail("ns_gl_finalize_weights: stft_fn.forward_basis is not a real DFT basis: the imaginary row of bin " + std::to_string(k) +
                        " holds an entry of magnitude above 1e-6");
      if (!(std::fabs(ib[(size_t)(bins + k) * fl + n]) <= 1e-9f))
        return api_fail("ns_gl_finalize_weights: stft_fn.inverse_basis is not the inverse of a real DFT basis: the imaginary row of bin " +
                        std::to_string(k) + " holds an entry of magnitude above 1e-9");
    }
  std::vector<float> img(h->ar.n, 0.f);
  auto packed_row = [&](int col) { return col == 0 ? 0 : col == 1 ? half : (col & 1) ? bins + col / 2 : col / 2; };
  for (int col = 0; col < fl; ++col) {
    const int src = packed_row(col);
    // forward: a weight row IS the basis row (melfront_api.hip).  inverse: weight row = output sample s of a frame, K index = packed
    // column: frames[m, s] = sum_col X[m, col] inverse_basis[row(col), s], the per-frame product of F.conv_transpose1d (stft.py:88-93)
    std::copy(fb.begin() + (size_t)src * fl, fb.begin() + (size_t)(src + 1) * fl, img.begin() + h->wf + (size_t)col * fl);
    for (int s = 0; s < fl; ++s) img[h->wi + (size_t)s * fl + col] = ib[(size_t)src * fl + s];
  }
  h->has_mel = h->weights.is_set(K_MEL);
  if (h->has_mel) std::copy(h->weights.data(K_MEL).begin(), h->weights.data(K_MEL).end(), img.begin() + h->mb);
  // squared periodic Hann window of win_length in float64, centre-padded to filter_length (audio_processing.py:55-57; the extra zero of an
  // odd difference goes to the right, as in librosa's pad_center)
  double* wsq = reinterpret_cast<double*>(&img[h->wsq]);
  const int lpad = (fl - h->win) / 2;
  for (int n = 0; n < fl; ++n) wsq[n] = 0.0;
  for (int n = 0; n < h->win; ++n) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * PI * (double)n / (double)h->win);
    wsq[lpad + n] = w * w;
  }
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(hipMemcpyAsync(h->arena, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st));
  NS_HIP(hipStreamSynchronize(st));  // img is a local
  h->weights.release();
  h->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ workspace
namespace {
struct Ws { float *rows, *spec, *X, *mag; };  // hop rows [B, S, hop]; packed spectrum [B, S, fl], reused for the frames [B, Tg, fl]; X [B, Tg, fl]
Ws carve(const ns_gl* h, void* base, int B, int T) {
  const size_t S = (size_t)T + h->kw - 1;
  Bump bp(base);
  Ws w;
  w.rows = bp.f((size_t)B * S * h->hop);
  w.spec = bp.f((size_t)B * S * h->fl);
  w.X = bp.f((size_t)B * T * h->fl);
  w.mag = bp.f((size_t)B * T * h->bins);
  return w;
}
}  // namespace

extern "C" size_t ns_gl_ws_bytes(const ns_gl* h, int B, int T_max) {
  if (!h || B <= 0 || T_max <= 0) return 256;
  const size_t S = (size_t)T_max + h->kw - 1;
  Bump bp(nullptr);
  bp.f((size_t)B * S * h->hop); bp.f((size_t)B * S * h->fl); bp.f((size_t)B * T_max * h->fl); bp.f((size_t)B * T_max * h->bins);
  return bp.off + 256;
}

static int check_ready(const ns_gl* h, const char* who) {
  if (!h) return api_fail(std::string(who) + ": null handle");
  if (!h->ready || !h->arena) return api_fail(std::string(who) + ": weights not finalized (ns_gl_finalize_weights)");
  return 0;
}

static int check_sizes(const ns_gl* h, int B, int T, const char* who) {
  if (B < 1 || T < 1) return api_fail(std::string(who) + ": B and the frame count must be >= 1");
  if ((long long)B * (T + h->kw - 1) >= (1ll << 31) / h->fl)
    return api_fail(std::string(who) + ": problem too large (B * rows * filter_length must stay below 2^31: split the batch)");
  if (B > 65535) return api_fail(std::string(who) + ": B must be at most 65535");
  return 0;
}

static int check_ws(const ns_gl* h, int B, int T, const void* ws, size_t ws_bytes, const char* who) {
  if (!ws) return api_fail(std::string(who) + ": null workspace");
  if (ws_bytes < ns_gl_ws_bytes(h, B, T)) return api_fail(std::string(who) + ": workspace too small (ns_gl_ws_bytes)");
  if ((uintptr_t)ws & 255) return api_fail(std::string(who) + ": workspace must be 256-byte aligned");
  return 0;
}

static int gemm(const float* X, int ldx, const float* W, float* Y, int M, int N, int Cin, int KW, int S, hipStream_t st) {
  ConvGemm p;
  memset(&p, 0, sizeof(p));
  p.X = X; p.ldx = ldx; p.W = W; p.Y = Y; p.ldy = N;
  p.M = M; p.N = N; p.Cin = Cin; p.KW = KW; p.pad = 0; p.S = S; p.act = ACT_NONE; p.epi = EPI_NONE;
  NS_HIP(launch_conv_gemm(p, st));
  return 0;
}

// forward STFT of hop rows [B, S, hop]: F.conv1d(stride = hop), stft.py:67-72 (the same call as ns_mel_forward's)
static int stft(const ns_gl* h, const float* rows, int B, int S, float* spec, hipStream_t st) {
  return gemm(rows, h->hop, h->P(h->wf), spec, B * S, h->fl, h->hop, h->kw, S, st);
}

// STFT.inverse from packed X [B * Tg, fl] (stft.py:88-120): the per-frame product as a plain GEMM (KW = 1), then the gather
static int inverse(const ns_gl* h, const float* X, const long long* lens, int drop, int B, int Tg, float* frames, float* wave, long long ld,
                   long long* wave_lens_out, hipStream_t st) {
  NS_TRY(gemm(X, h->fl, h->P(h->wi), frames, B * Tg, h->fl, h->fl, 1, Tg, st));
  NS_HIP(launch_gl_overlap_add(frames, lens, drop, B, Tg, h->fl, h->hop, reinterpret_cast<const double*>(h->P(h->wsq)), wave, ld, wave_lens_out, st));
  return 0;
}

// one iteration (audio_processing.py:80-81): transform without the clip, phase step, inverse.  wave_lens [B] holds n_b.
static int step(const ns_gl* h, const float* mag, const long long* lens, int drop, int B, int Tg, float* wave, long long ld, long long* wave_lens,
                const Ws& w, hipStream_t st) {
  const int S = Tg + h->kw - 1;
  const long long n_max = (long long)h->hop * (Tg - 1);
  NS_HIP(launch_mel_frame_rows(wave, ld, wave_lens, B, n_max, h->fl, h->hop, S, w.rows, nullptr, st, /*clip=*/false));
  NS_TRY(stft(h, w.rows, B, S, w.spec, st));
  NS_HIP(launch_gl_rephase(w.spec, mag, lens, drop, B, Tg, S, h->fl, h->hop, w.X, st));
  return inverse(h, w.X, lens, drop, B, Tg, w.spec, wave, ld, wave_lens, st);
}

static int check_wave(const ns_gl* h, int Tg, const float* wave, int64_t ld, const int64_t* wave_lens, const char* who) {
  if (!wave || !wave_lens) return api_fail(std::string(who) + ": null argument");
  if (ld < (int64_t)h->hop * (Tg - 1) || (ld & 3)) return api_fail(std::string(who) + ": ld_wave must be a multiple of 4 and at least hop_length * (frames - 1)");
  if ((uintptr_t)wave & 15) return api_fail(std::string(who) + ": wave must be 16-byte aligned");
  return 0;
}

static int run(ns_gl* h, const float* mag, const long long* lens, int drop, int B, int Tg, const float* angles, int n_iters, float* wave, int64_t ld,
               int64_t* wave_lens_out, const Ws& w, hipStream_t st) {
  long long* wl = reinterpret_cast<long long*>(wave_lens_out);
  NS_HIP(launch_gl_recombine(mag, angles, lens, drop, B, Tg, h->fl, h->hop, w.X, st));
  NS_TRY(inverse(h, w.X, lens, drop, B, Tg, w.spec, wave, ld, wl, st));
  for (int i = 0; i < n_iters; ++i) NS_TRY(step(h, mag, lens, drop, B, Tg, wave, ld, wl, w, st));
  return 0;
}

extern "C" int ns_gl_forward_mag(ns_gl* h, const float* mag, const int64_t* frame_lens, int B, int Tg, const float* angles, int n_iters, float* wave,
                                 int64_t ld_wave, int64_t* wave_lens_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ns_gl_forward_mag";
  NS_TRY(check_ready(h, who));
  if (B == 0) return 0;
  if (!mag || !frame_lens || !angles) return api_fail(std::string(who) + ": null argument");
  if (n_iters < 0) return api_fail(std::string(who) + ": n_iters must be >= 0");
  NS_TRY(check_sizes(h, B, Tg, who));
  NS_TRY(check_wave(h, Tg, wave, ld_wave, wave_lens_out, who));
  NS_TRY(check_ws(h, B, Tg, ws, ws_bytes, who));
  return run(h, mag, reinterpret_cast<const long long*>(frame_lens), 0, B, Tg, angles, n_iters, wave, ld_wave, wave_lens_out, carve(h, ws, B, Tg),
             (hipStream_t)stream);
}

extern "C" int ns_gl_forward(ns_gl* h, const float* mel, const int64_t* mel_lens, int B, int T, const float* angles, int n_iters, float* wave,
                             int64_t ld_wave, int64_t* wave_lens_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ns_gl_forward";
  NS_TRY(check_ready(h, who));
  if (!h->has_mel) return api_fail(std::string(who) + ": no mel_basis was loaded");
  if (B == 0) return 0;
  if (!mel || !mel_lens || !angles) return api_fail(std::string(who) + ": null argument");
  if (n_iters < 0) return api_fail(std::string(who) + ": n_iters must be >= 0");
  if (T < 2) return api_fail(std::string(who) + ": T must be >= 2 (the last mel frame is dropped, tools.py:28)");
  const int Tg = T - 1;
  NS_TRY(check_sizes(h, B, Tg, who));
  NS_TRY(check_wave(h, Tg, wave, ld_wave, wave_lens_out, who));
  NS_TRY(check_ws(h, B, T, ws, ws_bytes, who));
  hipStream_t st = (hipStream_t)stream;
  const long long* lens = reinterpret_cast<const long long*>(mel_lens);
  const Ws w = carve(h, ws, B, T);
  NS_HIP(launch_gl_mel_to_mag(mel, lens, 1, B, T, Tg, h->fl, h->hop, h->n_mel, h->scaling, h->P(h->mb), w.mag, st));
  return run(h, w.mag, lens, 1, B, Tg, angles, n_iters, wave, ld_wave, wave_lens_out, w, st);
}

extern "C" int ns_gl_transform(ns_gl* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int T, float* magnitude,
                               float* phase, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ns_gl_transform";
  NS_TRY(check_ready(h, who));
  if (B == 0) return 0;
  if (!wav || !wav_lens || !magnitude || !phase || n_max < 0 || ld_wav < n_max) return api_fail(std::string(who) + ": bad argument");
  const int64_t Tc64 = std::min<int64_t>(T, n_max / h->hop + 1);
  NS_TRY(check_sizes(h, B, (int)std::min<int64_t>(Tc64, 1 << 30), who));
  const int Tc = (int)Tc64, S = Tc + h->kw - 1;
  NS_TRY(check_ws(h, B, Tc, ws, ws_bytes, who));
  hipStream_t st = (hipStream_t)stream;
  const long long* lens = reinterpret_cast<const long long*>(wav_lens);
  const Ws w = carve(h, ws, B, Tc);
  NS_HIP(launch_mel_frame_rows(wav, ld_wav, lens, B, n_max, h->fl, h->hop, S, w.rows, nullptr, st, /*clip=*/false));
  NS_TRY(stft(h, w.rows, B, S, w.spec, st));
  NS_HIP(launch_gl_polar(w.spec, lens, n_max, B, S, T, h->fl, h->hop, magnitude, phase, st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ per-operator entry points
extern "C" int ns_gl_op_mel_to_mag(ns_gl* h, const float* mel, const int64_t* mel_lens, int B, int T, float* mag, void* stream) {
  const char* who = "ns_gl_op_mel_to_mag";
  NS_TRY(check_ready(h, who));
  if (!h->has_mel) return api_fail(std::string(who) + ": no mel_basis was loaded");
  if (!mel || !mel_lens || !mag || T < 2) return api_fail(std::string(who) + ": bad argument");
  NS_TRY(check_sizes(h, B, T - 1, who));
  NS_HIP(launch_gl_mel_to_mag(mel, reinterpret_cast<const long long*>(mel_lens), 1, B, T, T - 1, h->fl, h->hop, h->n_mel, h->scaling, h->P(h->mb), mag,
                              (hipStream_t)stream));
  return 0;
}

extern "C" int ns_gl_op_recombine(ns_gl* h, const float* mag, const float* angles, const int64_t* frame_lens, int B, int Tg, float* X, void* stream) {
  const char* who = "ns_gl_op_recombine";
  NS_TRY(check_ready(h, who));
  if (!mag || !angles || !frame_lens || !X || ((uintptr_t)X & 15)) return api_fail(std::string(who) + ": bad argument (X must be 16-byte aligned)");
  NS_TRY(check_sizes(h, B, Tg, who));
  NS_HIP(launch_gl_recombine(mag, angles, reinterpret_cast<const long long*>(frame_lens), 0, B, Tg, h->fl, h->hop, X, (hipStream_t)stream));
  return 0;
}

extern "C" int ns_gl_op_rephase(ns_gl* h, const float* Y, const float* mag, const int64_t* frame_lens, int B, int Tg, int S, float* X, void* stream) {
  const char* who = "ns_gl_op_rephase";
  NS_TRY(check_ready(h, who));
  if (!Y || !mag || !frame_lens || !X || S < Tg || (((uintptr_t)X | (uintptr_t)Y) & 15)) return api_fail(std::string(who) + ": bad argument (S >= frames; X and Y 16-byte aligned)");
  NS_TRY(check_sizes(h, B, std::max(Tg, S - h->kw + 1), who));
  NS_HIP(launch_gl_rephase(Y, mag, reinterpret_cast<const long long*>(frame_lens), 0, B, Tg, S, h->fl, h->hop, X, (hipStream_t)stream));
  return 0;
}

extern "C" int ns_gl_op_inverse(ns_gl* h, const float* X, const int64_t* frame_lens, int B, int Tg, float* wave, int64_t ld_wave, int64_t* wave_lens_out,
                                void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ns_gl_op_inverse";
  NS_TRY(check_ready(h, who));
  if (!X || !frame_lens || ((uintptr_t)X & 15)) return api_fail(std::string(who) + ": bad argument (X must be 16-byte aligned)");
  NS_TRY(check_sizes(h, B, Tg, who));
  NS_TRY(check_wave(h, Tg, wave, ld_wave, wave_lens_out, who));
  NS_TRY(check_ws(h, B, Tg, ws, ws_bytes, who));
  return inverse(h, X, reinterpret_cast<const long long*>(frame_lens), 0, B, Tg, carve(h, ws, B, Tg).spec, wave, ld_wave,
                 reinterpret_cast<long long*>(wave_lens_out), (hipStream_t)stream);
}

extern "C" int ns_gl_op_frame_rows(ns_gl* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int S, float* rows,
                                   void* stream) {
  const char* who = "ns_gl_op_frame_rows";
  if (!h || !wav || !wav_lens || !rows || B <= 0 || S < h->kw || n_max < 0 || ld_wav < n_max) return api_fail(std::string(who) + ": bad argument");
  if ((uintptr_t)rows & 15) return api_fail(std::string(who) + ": rows must be 16-byte aligned");
  NS_TRY(check_sizes(h, B, S - h->kw + 1, who));
  NS_HIP(launch_mel_frame_rows(wav, ld_wav, reinterpret_cast<const long long*>(wav_lens), B, n_max, h->fl, h->hop, S, rows, nullptr, (hipStream_t)stream,
                               /*clip=*/false));
  return 0;
}

extern "C" int ns_gl_op_step(ns_gl* h, const float* mag, const int64_t* frame_lens, int B, int Tg, float* wave, int64_t ld_wave, int64_t* wave_lens_out,
                             void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ns_gl_op_step";
  NS_TRY(check_ready(h, who));
  if (!mag || !frame_lens) return api_fail(std::string(who) + ": null argument");
  NS_TRY(check_sizes(h, B, Tg, who));
  NS_TRY(check_wave(h, Tg, wave, ld_wave, wave_lens_out, who));
  NS_TRY(check_ws(h, B, Tg, ws, ws_bytes, who));
  hipStream_t st = (hipStream_t)stream;
  const long long* lens = reinterpret_cast<const long long*>(frame_lens);
  long long* wl = reinterpret_cast<long long*>(wave_lens_out);
  NS_HIP(launch_gl_wave_lens(lens, 0, B, Tg, h->fl, h->hop, wl, st));
  return step(h, mag, lens, 0, B, Tg, wave, ld_wave, wl, carve(h, ws, B, Tg), st);
}
