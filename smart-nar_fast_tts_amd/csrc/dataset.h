// Device-resident training set (include/nar_fs2.h ns_ds_*): what dataset.hip (the kernel) and dataset_api.hip
// (the host entry points, ns_ds_host_gather among them) share.  A batch's outputs are one flat list of work items:
//   [0, w_mel)            one 16-byte group (four floats) of mels [B, Tmax, n_mel]
//   [w_mel, w_pitch)      one element of pitches [B, Pmax]
//   [w_pitch, w_energy)   one element of energies [B, Emax]
//   [w_energy, w_text)    one element of texts [B, Lmax]
//   [w_text, w_total)     utterance b's speaker, src_len and mel_len
// ds_mel_item and ds_tail_item are __host__ __device__: the kernel and the host gather compile this text, so the two cannot drift.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nar_fs2.h"

namespace ns {

constexpr int DS_BLOCK = 256;                 // threads of a workgroup: one work item each a turn
constexpr int DS_GRID_CAP = NS_DS_GRID_CAP;   // workgroups of a launch at most; they loop over the items beyond

struct DsArgs {
  ns_ds_store s;
  ns_ds_batch o;
  const int32_t* order;  // the batch's first entry: order + first
  uint32_t groups;       // n_mel / 4
  int64_t w_mel, w_pitch, w_energy, w_text, w_total;  // the ends of the five item ranges
};

typedef uint32_t DsQuad __attribute__((ext_vector_type(4)));  // 16 aligned bytes moved as they are (no float is ever formed)

// an order entry outside [0, N) is an utterance of length 0: nothing is read for it
__host__ __device__ inline int ds_utt(const DsArgs& a, uint32_t b) {
  const int32_t i = a.order[b];
  return (i >= 0 && i < a.s.N) ? i : -1;
}

// one element of a padded [B, cap] output from a ragged fp32 or int32 array: the store's dword below the utterance's length (and
// inside the array), else 0
__host__ __device__ inline uint32_t ds_dword(const DsArgs& a, uint32_t r, uint32_t cap, const void* src, const int64_t* off, const int32_t* len,
                                             int64_t elems) {
  const uint32_t b = r / cap, p = r - b * cap;
  const int i = ds_utt(a, b);
  if (i < 0 || (int64_t)p >= (int64_t)len[i]) return 0u;
  const int64_t e = off[i] + (int64_t)p;
  return (e >= 0 && e < elems) ? ((const uint32_t*)src)[e] : 0u;
}

// item r of the mel range: one 16-byte group of mels
__host__ __device__ inline void ds_mel_item(const DsArgs& a, uint32_t r) {
  const uint32_t per = (uint32_t)a.o.Tmax * a.groups;
  const uint32_t b = r / per, q = r - b * per, t = q / a.groups, g = q - t * a.groups;
  const int i = ds_utt(a, b);
  DsQuad v = (DsQuad)(0u);
  if (i >= 0 && (int64_t)t < (int64_t)a.s.mel_len[i]) {
    const int64_t row = a.s.mel_off[i] + (int64_t)t;
    if (row >= 0 && row < a.s.mel_rows) v = ((const DsQuad*)a.s.mel)[row * (int64_t)a.groups + (int64_t)g];
  }
  ((DsQuad*)a.o.mels)[r] = v;
}

// item w of the ranges behind the mel's, w in [w_mel, w_total)
__host__ __device__ inline void ds_tail_item(const DsArgs& a, int64_t w) {
  if (w < a.w_pitch) {
    const uint32_t r = (uint32_t)(w - a.w_mel);
    ((uint32_t*)a.o.pitches)[r] = ds_dword(a, r, (uint32_t)a.o.Pmax, a.s.pitch, a.s.pitch_off, a.s.pitch_len, a.s.pitch_elems);
  } else if (w < a.w_energy) {
    const uint32_t r = (uint32_t)(w - a.w_pitch);
    ((uint32_t*)a.o.energies)[r] = ds_dword(a, r, (uint32_t)a.o.Emax, a.s.energy, a.s.energy_off, a.s.energy_len, a.s.energy_elems);
  } else if (w < a.w_text) {
    const uint32_t r = (uint32_t)(w - a.w_energy);
    a.o.texts[r] = (int64_t)(int32_t)ds_dword(a, r, (uint32_t)a.o.Lmax, a.s.text, a.s.text_off, a.s.text_len, a.s.text_elems);
  } else if (w < a.w_total) {
    const uint32_t b = (uint32_t)(w - a.w_text);
    const int i = ds_utt(a, b);
    a.o.speakers[b] = i < 0 ? 0 : (int64_t)a.s.speaker[i];
    a.o.src_lens[b] = i < 0 ? 0 : (int64_t)a.s.text_len[i];
    a.o.mel_lens[b] = i < 0 ? 0 : (int64_t)a.s.mel_len[i];
  }
}

// the item ranges of a batch; every output is below 2^31 elements (the entry points refuse the rest), so an index inside a range
// fits 32 bits
inline DsArgs ds_args(const ns_ds_store& s, const ns_ds_batch& o, const int32_t* order_first) {
  DsArgs a;
  a.s = s; a.o = o; a.order = order_first;
  a.groups = (uint32_t)(s.n_mel / 4);
  a.w_mel = (int64_t)o.B * o.Tmax * (int64_t)a.groups;
  a.w_pitch = a.w_mel + (int64_t)o.B * o.Pmax;
  a.w_energy = a.w_pitch + (int64_t)o.B * o.Emax;
  a.w_text = a.w_energy + (int64_t)o.B * o.Lmax;
  a.w_total = a.w_text + (int64_t)o.B;
  return a;
}

// k_ds_gather over the items of a: exactly one launch of min(ceil(w_total / DS_BLOCK), grid_cap) workgroups
hipError_t launch_ds_gather(const DsArgs& a, int grid_cap, hipStream_t st);

}  // namespace ns
