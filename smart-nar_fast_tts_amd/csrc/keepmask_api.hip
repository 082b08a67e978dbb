// C-ABI of the dropout keep-mask generator (include/nar_fs2.h ns_km_*).  No handle: the table is the caller's
// (planned on the host by ns_km_plan, uploaded by the caller), the arena is the caller's, and the generator's state is the two integers
// the caller passes.  Host-side only; every argument is validated before the first HIP call.  ns_km_op_philox and ns_km_host_draw run
// the same inline functions the kernel compiles (keepmask.h) on the host and touch no GPU.
#include "keepmask.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_km_mask) == 16, "ns_km_mask layout");

namespace {
thread_local int t_launches = 0;

constexpr uint64_t KM_MAX_N = 1ull << 34;  // a block index is 32 bits and a block is four elements

int check_count(const std::string& w, int n_masks) {
  if (n_masks < 1 || n_masks > KM_MAX_MASKS)
    return api_fail(w + "n_masks must lie in [1, " + std::to_string(KM_MAX_MASKS) + "], got " + std::to_string(n_masks));
  return 0;
}

int check_mask(const std::string& w, int i, uint64_t n, uint32_t thr) {
  if (n == 0) return api_fail(w + "masks[" + std::to_string(i) + "].n must be positive");
  if (n >= KM_MAX_N) return api_fail(w + "masks[" + std::to_string(i) + "].n must stay below 2^34");
  if (thr == 0) return api_fail(w + "masks[" + std::to_string(i) + "].thr must not be 0 (nothing would be kept)");
  return 0;
}
}  // namespace

extern "C" int ns_km_abi_version(void) { return NS_KM_ABI_VERSION; }
extern "C" int ns_km_last_launches(void) { return t_launches; }

extern "C" int ns_km_threshold(double p, uint32_t* thr) {
  const std::string w = "ns_km_threshold: ";
  if (!thr) return api_fail(w + "null argument");
  if (!(p > 0.0 && p < 1.0)) return api_fail(w + "p must lie in (0, 1)");
  const double t = std::floor((1.0 - p) * 4294967296.0);
  if (t < 1.0) return api_fail(w + "p is too close to 1: the threshold would be 0 (nothing would be kept)");
  if (t >= 4294967296.0) return api_fail(w + "p is too close to 0: the threshold does not fit 32 bits");
  *thr = (uint32_t)t;
  return 0;
}

extern "C" size_t ns_km_table_bytes(int n_masks) {
  if (check_count("ns_km_table_bytes: ", n_masks)) return 0;
  return (size_t)(n_masks + 1) * sizeof(KmEntry);
}

extern "C" int ns_km_plan(const ns_km_mask* masks, int n_masks, void* table_host, size_t table_bytes, uint64_t* arena_bytes) {
  const std::string w = "ns_km_plan: ";
  if (!masks || !table_host || !arena_bytes) return api_fail(w + "null argument");
  NS_TRY(check_count(w, n_masks));
  for (int i = 0; i < n_masks; ++i) NS_TRY(check_mask(w, i, masks[i].n, masks[i].thr));
  if (table_bytes < (size_t)(n_masks + 1) * sizeof(KmEntry)) return api_fail(w + "table too small (ns_km_table_bytes)");
  uint64_t off = 0, chunks = 0;
  for (int i = 0; i <= n_masks; ++i) {
    KmEntry e;
    memset(&e, 0, sizeof(e));
    e.offset = off; e.chunk_begin = chunks;
    if (i < n_masks) {
      e.n = masks[i].n; e.stream = masks[i].stream; e.thr = masks[i].thr;
      off += (e.n + 15) & ~(uint64_t)15;
      chunks += (e.n + KM_CHUNK - 1) / KM_CHUNK;
    }
    memcpy((char*)table_host + (size_t)i * sizeof(KmEntry), &e, sizeof(e));  // (the caller's buffer need not be aligned)
  }
  *arena_bytes = off;
  return 0;
}

extern "C" int ns_km_draw(const void* table_dev, int n_masks, uint64_t seed, uint64_t call, void* arena, size_t arena_bytes, void* stream) {
  const std::string w = "ns_km_draw: ";
  t_launches = 0;
  if (!table_dev || !arena) return api_fail(w + "null argument");
  NS_TRY(check_count(w, n_masks));
  NS_TRY(check_aligned(w, {{"the table", table_dev, 8}, {"the arena", arena}}));
  // the table is on the device and is not read here: what the host can refuse is an arena no plan of n_masks masks fits (a slot is at
  // least 16 bytes); past that the kernel itself makes no store that would end behind arena_bytes
  if (arena_bytes < (size_t)n_masks * 16) return api_fail(w + "arena too small: " + std::to_string(n_masks) + " masks need at least " +
                                                          std::to_string((size_t)n_masks * 16) + " bytes (ns_km_plan)");
  NS_HIP(launch_km_draw((const KmEntry*)table_dev, n_masks, seed, call, (uint8_t*)arena, (uint64_t)arena_bytes, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_km_op_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  if (!ctr || !key || !out) return api_fail("ns_km_op_philox: null argument");
  const KmWords r = km_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  memcpy(out, r.w, sizeof(r.w));
  return 0;
}

extern "C" int ns_km_host_draw(const void* table_host, int n_masks, uint64_t seed, uint64_t call, void* arena_host, size_t arena_bytes) {
  const std::string w = "ns_km_host_draw: ";
  t_launches = 0;
  if (!table_host || !arena_host) return api_fail(w + "null argument");
  NS_TRY(check_count(w, n_masks));
  std::vector<KmEntry> t((size_t)n_masks + 1);
  memcpy(t.data(), table_host, t.size() * sizeof(KmEntry));
  uint64_t off = 0;
  for (int i = 0; i < n_masks; ++i) {  // the table must be a plan's: slots in order, back to back
    NS_TRY(check_mask(w, i, t[i].n, t[i].thr));
    if (t[i].offset != off) return api_fail(w + "the table is not one ns_km_plan wrote (slot " + std::to_string(i) + " is out of place)");
    off += (t[i].n + 15) & ~(uint64_t)15;
  }
  if ((uint64_t)arena_bytes < off) return api_fail(w + "arena too small: " + std::to_string(off) + " bytes needed (ns_km_plan)");
  for (int i = 0; i < n_masks; ++i) {
    const uint64_t slot = (t[i].n + 15) & ~(uint64_t)15;
    for (uint64_t e0 = 0; e0 < slot; e0 += KM_THREAD_ELEMS) {
      uint32_t v[4];
      km_draw16(e0, t[i].n, t[i].stream, t[i].thr, seed, call, v);
      uint8_t* dst = (uint8_t*)arena_host + t[i].offset + e0;
      for (int b = 0; b < KM_THREAD_ELEMS; ++b) dst[b] = (uint8_t)(v[b >> 2] >> (8 * (b & 3)));  // (the device's byte order, on any host)
    }
  }
  return 0;
}
