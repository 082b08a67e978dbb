// C-ABI of the device-resident training set (include/nar_fs2.h ns_ds_*).  No handle: the store, the tables and
// the outputs are the caller's.  Host-side only; every argument is validated before the first HIP call, the per-batch maxima from the
// HOST length vectors the caller passes (the device is not read).  ns_ds_host_gather runs the same inline function the kernel compiles
// (dataset.h) on host arrays and touches no GPU.
#include "dataset.h"
#include "train_api.h"

using namespace ns;

namespace {
thread_local int t_launches = 0;

constexpr int64_t DS_MAX_OUT = (int64_t)1 << 31;  // elements of one output, exclusive: an index inside an output fits 32 bits

inline int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

int check_geometry(const std::string& w, int N, int n_mel) {
  if (N < 1) return api_fail(w + "N must be positive, got " + std::to_string(N));
  if (n_mel < 4 || n_mel > 128 || n_mel % 4 != 0) return api_fail(w + "n_mel must be a multiple of 4 in [4, 128], got " + std::to_string(n_mel));
  return 0;
}

int check_lens(const std::string& w, const ns_ds_lens* lens) {
  if (!lens || !lens->text || !lens->mel || !lens->pitch || !lens->energy) return api_fail(w + "null argument (lens)");
  return 0;
}

// everything ns_ds_gather and ns_ds_host_gather refuse alike; *a: the launch's arguments
int check_batch(const std::string& w, const ns_ds_store* s, const ns_ds_lens* lens, const int32_t* order_host, int64_t order_len, int64_t first,
                const ns_ds_batch* o) {
  const int align = 16;
  if (!s || !o || !order_host) return api_fail(w + "null argument");
  NS_TRY(check_lens(w, lens));
  if (!s->mel || !s->pitch || !s->energy || !s->text || !s->speaker || !s->mel_off || !s->pitch_off || !s->energy_off || !s->text_off ||
      !s->text_len || !s->mel_len || !s->pitch_len || !s->energy_len)
    return api_fail(w + "null pointer in the store");
  if (!o->mels || !o->pitches || !o->energies || !o->texts || !o->speakers || !o->src_lens || !o->mel_lens)
    return api_fail(w + "null pointer in the batch");
  NS_TRY(check_geometry(w, s->N, s->n_mel));
  if (o->B < 1) return api_fail(w + "B must be positive, got " + std::to_string(o->B));
  if (first < 0 || order_len < 0 || first > order_len || (int64_t)o->B > order_len - first)
    return api_fail(w + "first + B must not pass the order's length: first " + std::to_string(first) + ", B " + std::to_string(o->B) + ", order_len " +
                    std::to_string(order_len));
  if (s->mel_rows < 1 || s->pitch_elems < 1 || s->energy_elems < 1 || s->text_elems < 1)
    return api_fail(w + "the store's sizes must be positive (ns_ds_plan)");
  NS_TRY(check_aligned(w, {{"store->mel", s->mel, align}, {"store->pitch", s->pitch, align}, {"store->energy", s->energy, align},
                           {"store->text", s->text, align}, {"store->speaker", s->speaker, 4}, {"store->mel_off", s->mel_off, 8},
                           {"store->pitch_off", s->pitch_off, 8}, {"store->energy_off", s->energy_off, 8}, {"store->text_off", s->text_off, 8},
                           {"store->text_len", s->text_len, 4}, {"store->mel_len", s->mel_len, 4}, {"store->pitch_len", s->pitch_len, 4},
                           {"store->energy_len", s->energy_len, 4}, {"out->mels", o->mels, align}, {"out->pitches", o->pitches, 4},
                           {"out->energies", o->energies, 4}, {"out->texts", o->texts, 8}, {"out->speakers", o->speakers, 8},
                           {"out->src_lens", o->src_lens, 8}, {"out->mel_lens", o->mel_lens, 8}}));
  int32_t mt = 0, mp = 0, me = 0, ml = 0;
  for (int b = 0; b < o->B; ++b) {
    const int32_t i = order_host[first + b];
    if (i < 0 || i >= s->N)
      return api_fail(w + "order[" + std::to_string(first + b) + "] = " + std::to_string(i) + " is outside [0, N = " + std::to_string(s->N) + ")");
    mt = std::max(mt, lens->mel[i]); mp = std::max(mp, lens->pitch[i]); me = std::max(me, lens->energy[i]); ml = std::max(ml, lens->text[i]);
  }
  const struct { const char* name; int32_t got, need; } caps[4] = {{"Tmax", o->Tmax, mt}, {"Pmax", o->Pmax, mp}, {"Emax", o->Emax, me}, {"Lmax", o->Lmax, ml}};
  for (const auto& c : caps)
    if (c.got < 1 || c.got < c.need)
      return api_fail(w + c.name + " = " + std::to_string(c.got) + " is below the batch's own maximum " + std::to_string(std::max(c.need, 1)));
  const int64_t B = o->B;
  if (B * o->Tmax * s->n_mel >= DS_MAX_OUT || B * o->Pmax >= DS_MAX_OUT || B * o->Emax >= DS_MAX_OUT || B * o->Lmax >= DS_MAX_OUT)
    return api_fail(w + "every output must stay below 2^31 elements");
  return 0;
}

int gather(const std::string& w, const ns_ds_store* s, const ns_ds_lens* lens, const int32_t* order_dev, const int32_t* order_host, int64_t order_len,
           int64_t first, const ns_ds_batch* o, int grid_cap, void* stream) {
  t_launches = 0;
  if (!order_dev) return api_fail(w + "null argument");
  NS_TRY(check_aligned(w, {{"order_dev", order_dev, 4}}));
  if (grid_cap < 1 || grid_cap > DS_GRID_CAP)
    return api_fail(w + "grid_cap must lie in [1, " + std::to_string(DS_GRID_CAP) + "], got " + std::to_string(grid_cap));
  NS_TRY(check_batch(w, s, lens, order_host, order_len, first, o));
  NS_HIP(launch_ds_gather(ds_args(*s, *o, order_dev + first), grid_cap, (hipStream_t)stream));
  ++t_launches;
  return 0;
}
}  // namespace

extern "C" int ns_ds_abi_version(void) { return NS_DS_ABI_VERSION; }
extern "C" int ns_ds_last_launches(void) { return t_launches; }

extern "C" int ns_ds_plan(const ns_ds_lens* lens, int N, int n_mel, const ns_ds_offsets* off, uint64_t bytes[4]) {
  const std::string w = "ns_ds_plan: ";
  t_launches = 0;
  if (!off || !bytes || !off->mel || !off->pitch || !off->energy || !off->text) return api_fail(w + "null argument");
  NS_TRY(check_lens(w, lens));
  NS_TRY(check_geometry(w, N, n_mel));
  const int32_t* len[4] = {lens->mel, lens->pitch, lens->energy, lens->text};
  const char* name[4] = {"mel", "pitch", "energy", "text"};
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < N; ++i)
      if (len[k][i] < 1) return api_fail(w + "lens->" + name[k] + "[" + std::to_string(i) + "] must be positive, got " + std::to_string(len[k][i]));
  int64_t* out[4] = {off->mel, off->pitch, off->energy, off->text};
  for (int k = 0; k < 4; ++k) {
    int64_t at = 0;
    for (int i = 0; i < N; ++i) {
      out[k][i] = at;
      at += k == 0 ? (int64_t)len[k][i] : round4(len[k][i]);  // mel rows are 4 n_mel bytes, a multiple of 16, as they are
    }
    out[k][N] = at;
    bytes[k] = (uint64_t)at * (k == 0 ? (uint64_t)n_mel * 4u : 4u);
  }
  return 0;
}

extern "C" int ns_ds_gather(const ns_ds_store* store, const ns_ds_lens* lens, const int32_t* order_dev, const int32_t* order_host, int64_t order_len,
                            int64_t first, const ns_ds_batch* out, void* stream) {
  return gather("ns_ds_gather: ", store, lens, order_dev, order_host, order_len, first, out, DS_GRID_CAP, stream);
}

extern "C" int ns_ds_op_gather(const ns_ds_store* store, const ns_ds_lens* lens, const int32_t* order_dev, const int32_t* order_host,
                               int64_t order_len, int64_t first, const ns_ds_batch* out, int grid_cap, void* stream) {
  return gather("ns_ds_op_gather: ", store, lens, order_dev, order_host, order_len, first, out, grid_cap, stream);
}

extern "C" int ns_ds_host_gather(const ns_ds_store* store, const ns_ds_lens* lens, const int32_t* order_host, int64_t order_len, int64_t first,
                                 const ns_ds_batch* out) {
  const std::string w = "ns_ds_host_gather: ";
  t_launches = 0;
  NS_TRY(check_batch(w, store, lens, order_host, order_len, first, out));
  const ns_ds_store& s = *store;
  // the tables must be a plan's for these lengths: every entry, and the stated sizes cover the last row
  const int32_t* len[4] = {lens->mel, lens->pitch, lens->energy, lens->text};
  const int64_t* off[4] = {s.mel_off, s.pitch_off, s.energy_off, s.text_off};
  const int32_t* copy[4] = {s.mel_len, s.pitch_len, s.energy_len, s.text_len};
  const int64_t size[4] = {s.mel_rows, s.pitch_elems, s.energy_elems, s.text_elems};
  const char* name[4] = {"mel", "pitch", "energy", "text"};
  for (int k = 0; k < 4; ++k) {
    int64_t at = 0;
    for (int i = 0; i <= s.N; ++i) {
      if (off[k][i] != at)
        return api_fail(w + "store->" + name[k] + "_off is not one ns_ds_plan wrote (entry " + std::to_string(i) + " is " + std::to_string(off[k][i]) +
                        ", the plan's is " + std::to_string(at) + ")");
      if (i == s.N) break;
      if (len[k][i] < 1 || copy[k][i] != len[k][i])
        return api_fail(w + "store->" + name[k] + "_len[" + std::to_string(i) + "] is not the positive length lens states");
      at += k == 0 ? (int64_t)len[k][i] : round4(len[k][i]);
    }
    if (size[k] < at) return api_fail(w + "store->" + name[k] + " is stated shorter than its table's last row (ns_ds_plan)");
  }
  const DsArgs a = ds_args(s, *out, order_host + first);
  for (int64_t i = 0; i < a.w_mel; ++i) ds_mel_item(a, (uint32_t)i);
  for (int64_t i = a.w_mel; i < a.w_total; ++i) ds_tail_item(a, i);
  return 0;
}
