/* A plain-C caller of the ns_ds_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, every refusal
 * must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call), and ns_ds_plan + ns_ds_host_gather must
 * give the padded batch of a three-utterance store written out by hand.  Run by tests/test_dataset_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef int (*plan_fn)(const ns_ds_lens*, int, int, const ns_ds_offsets*, uint64_t*);
typedef int (*gather_fn)(const ns_ds_store*, const ns_ds_lens*, const int32_t*, const int32_t*, int64_t, int64_t, const ns_ds_batch*, void*);
typedef int (*op_gather_fn)(const ns_ds_store*, const ns_ds_lens*, const int32_t*, const int32_t*, int64_t, int64_t, const ns_ds_batch*, int, void*);
typedef int (*host_gather_fn)(const ns_ds_store*, const ns_ds_lens*, const int32_t*, int64_t, int64_t, const ns_ds_batch*);

#define NU 3
#define NMEL 4

int main(int argc, char** argv) {
  void* so;
  /* utterance i: L = text_len[i] phonemes, T = mel_len[i] frames; pitch is phoneme level, energy frame level */
  int32_t text_len[NU] = {2, 5, 1}, mel_len[NU] = {3, 1, 6}, order[4] = {2, 0, 2, 1};
  int64_t off[4][NU + 1];
  uint64_t bytes[4];
  ns_ds_lens lens, bad_lens;
  ns_ds_offsets offs, bad_offs;
  ns_ds_store s, bs;
  ns_ds_batch o, bo;
  float *mel, *pitch, *energy, *mels, *pitches, *energies;
  int32_t *text, speaker[NU] = {7, 8, 9}, zero_len[NU] = {2, 0, 1};
  int64_t *texts, small[3 * 3], saved;
  void* dev = (void*)0x1000000; /* a made-up device address: never dereferenced */
  int i, b, t, c;
  last_error_fn last_error; version_fn version, launches; plan_fn plan; gather_fn gather; op_gather_fn op_gather; host_gather_fn host_gather;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_ds_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_ds_last_launches");
  *(void**)(&plan) = dlsym(so, "ns_ds_plan");
  *(void**)(&gather) = dlsym(so, "ns_ds_gather");
  *(void**)(&op_gather) = dlsym(so, "ns_ds_op_gather");
  *(void**)(&host_gather) = dlsym(so, "ns_ds_host_gather");
  if (!last_error || !version || !launches || !plan || !gather || !op_gather || !host_gather) { printf("missing symbol\n"); return 4; }
  if (version() != NS_DS_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* ns_ds_plan */
  lens.text = text_len; lens.mel = mel_len; lens.pitch = text_len; lens.energy = mel_len;
  offs.mel = off[0]; offs.pitch = off[1]; offs.energy = off[2]; offs.text = off[3];
  if (plan(0, NU, NMEL, &offs, bytes) == 0 || !strstr(last_error(), "null argument")) return 10;
  if (plan(&lens, NU, NMEL, 0, bytes) == 0 || !strstr(last_error(), "null argument")) return 11;
  if (plan(&lens, NU, NMEL, &offs, 0) == 0 || !strstr(last_error(), "null argument")) return 12;
  bad_offs = offs; bad_offs.energy = 0;
  if (plan(&lens, NU, NMEL, &bad_offs, bytes) == 0 || !strstr(last_error(), "null argument")) return 13;
  bad_lens = lens; bad_lens.pitch = 0;
  if (plan(&bad_lens, NU, NMEL, &offs, bytes) == 0 || !strstr(last_error(), "null argument")) return 14;
  if (plan(&lens, 0, NMEL, &offs, bytes) == 0 || !strstr(last_error(), "N must be positive")) return 15;
  if (plan(&lens, NU, 6, &offs, bytes) == 0 || !strstr(last_error(), "n_mel must be a multiple of 4 in [4, 128]")) return 16;
  if (plan(&lens, NU, 132, &offs, bytes) == 0 || !strstr(last_error(), "n_mel must be a multiple of 4 in [4, 128]")) return 17;
  if (plan(&lens, NU, 0, &offs, bytes) == 0 || !strstr(last_error(), "n_mel must be a multiple of 4")) return 18;
  bad_lens = lens; bad_lens.energy = zero_len;
  if (plan(&bad_lens, NU, NMEL, &offs, bytes) == 0 || !strstr(last_error(), "lens->energy[1] must be positive")) return 19;
  if (plan(&lens, NU, NMEL, &offs, bytes) != 0) return 20;
  if (off[0][0] != 0 || off[0][1] != 3 || off[0][2] != 4 || off[0][3] != 10 || bytes[0] != 10 * NMEL * 4) return 21; /* mel: rows, as they are */
  if (off[1][0] != 0 || off[1][1] != 4 || off[1][2] != 12 || off[1][3] != 16 || bytes[1] != 64) return 22;           /* pitch: L = 2, 5, 1 in slots of 4, 8, 4 */
  if (off[2][0] != 0 || off[2][1] != 4 || off[2][2] != 8 || off[2][3] != 16 || bytes[2] != 64) return 23;            /* energy: T = 3, 1, 6 in slots of 4, 4, 8 */
  if (memcmp(off[3], off[1], sizeof(off[1])) != 0 || bytes[3] != 64) return 24;
  /* the store: element e of utterance i is 100 i + e (+ 1000 column for the mel, + 0.5 pitch, + 0.25 energy); slot padding is -1 */
  mel = (float*)malloc(bytes[0]); pitch = (float*)malloc(bytes[1]); energy = (float*)malloc(bytes[2]); text = (int32_t*)malloc(bytes[3]);
  if (!mel || !pitch || !energy || !text) return 6;
  for (i = 0; i < 16; ++i) { pitch[i] = -1.f; energy[i] = -1.f; text[i] = -1; }
  for (i = 0; i < NU; ++i) {
    for (t = 0; t < mel_len[i]; ++t) {
      for (c = 0; c < NMEL; ++c) mel[(off[0][i] + t) * NMEL + c] = (float)(100 * i + t + 1000 * c);
      energy[off[2][i] + t] = (float)(100 * i + t) + 0.25f;
    }
    for (t = 0; t < text_len[i]; ++t) { pitch[off[1][i] + t] = (float)(100 * i + t) + 0.5f; text[off[3][i] + t] = 100 * i + t + 1; }
  }
  memset(&s, 0, sizeof(s));
  s.mel = mel; s.pitch = pitch; s.energy = energy; s.text = text; s.speaker = speaker;
  s.mel_off = off[0]; s.pitch_off = off[1]; s.energy_off = off[2]; s.text_off = off[3];
  s.text_len = text_len; s.mel_len = mel_len; s.pitch_len = text_len; s.energy_len = mel_len;
  s.mel_rows = off[0][NU]; s.pitch_elems = off[1][NU]; s.energy_elems = off[2][NU]; s.text_elems = off[3][NU];
  s.N = NU; s.n_mel = NMEL;
  /* the batch order[1 .. 4) = utterances 0, 2, 1, one column wider than it needs on every axis */
  memset(&o, 0, sizeof(o));
  o.B = 3; o.Tmax = 7; o.Pmax = 6; o.Emax = 7; o.Lmax = 6;
  mels = (float*)malloc(sizeof(float) * 3 * 7 * NMEL); pitches = (float*)malloc(sizeof(float) * 3 * 6); energies = (float*)malloc(sizeof(float) * 3 * 7);
  texts = (int64_t*)malloc(sizeof(int64_t) * 3 * 6);
  if (!mels || !pitches || !energies || !texts) return 6;
  memset(mels, 0xFF, sizeof(float) * 3 * 7 * NMEL); memset(pitches, 0xFF, sizeof(float) * 18); memset(energies, 0xFF, sizeof(float) * 21);
  memset(texts, 0xFF, sizeof(int64_t) * 18); memset(small, 0xFF, sizeof(small));
  o.mels = mels; o.pitches = pitches; o.energies = energies; o.texts = texts; o.speakers = small; o.src_lens = small + 3; o.mel_lens = small + 6;
  /* refusals shared by the three gathers, through the host one */
  if (host_gather(0, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "null argument")) return 30;
  if (host_gather(&s, 0, order, 4, 1, &o) == 0 || !strstr(last_error(), "null argument")) return 31;
  if (host_gather(&s, &lens, 0, 4, 1, &o) == 0 || !strstr(last_error(), "null argument")) return 32;
  if (host_gather(&s, &lens, order, 4, 1, 0) == 0 || !strstr(last_error(), "null argument")) return 33;
  bs = s; bs.energy = 0;
  if (host_gather(&bs, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "null pointer in the store")) return 34;
  bo = o; bo.mel_lens = 0;
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "null pointer in the batch")) return 35;
  bs = s; bs.mel = mel + 1;
  if (host_gather(&bs, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "store->mel must be 16-byte aligned")) return 36;
  bo = o; bo.texts = (int64_t*)((char*)texts + 4);
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "out->texts must be 8-byte aligned")) return 37;
  bs = s; bs.n_mel = 6;
  if (host_gather(&bs, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "n_mel must be a multiple of 4 in [4, 128]")) return 38;
  bs = s; bs.N = 0;
  if (host_gather(&bs, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "N must be positive")) return 39;
  bo = o; bo.B = 0;
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "B must be positive")) return 40;
  if (host_gather(&s, &lens, order, 4, 2, &o) == 0 || !strstr(last_error(), "first + B must not pass the order's length")) return 41;
  if (host_gather(&s, &lens, order, 4, -1, &o) == 0 || !strstr(last_error(), "first + B must not pass")) return 42;
  bo = o; bo.Tmax = 5;
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "Tmax = 5 is below the batch's own maximum 6")) return 43;
  bo = o; bo.Pmax = 4;
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "Pmax = 4 is below the batch's own maximum 5")) return 44;
  bo = o; bo.Emax = 0;
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "Emax = 0 is below the batch's own maximum 6")) return 45;
  bo = o; bo.Lmax = 4;
  if (host_gather(&s, &lens, order, 4, 1, &bo) == 0 || !strstr(last_error(), "Lmax = 4 is below the batch's own maximum 5")) return 46;
  bo = o; bo.B = 1; bo.Tmax = 1 << 29; /* 2^29 rows of 4 floats */
  if (host_gather(&s, &lens, order, 4, 0, &bo) == 0 || !strstr(last_error(), "every output must stay below 2^31 elements")) return 47;
  order[3] = 3;
  if (host_gather(&s, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "order[3] = 3 is outside [0, N = 3)")) return 48;
  order[3] = 1;
  saved = off[1][2]; off[1][2] = 9; /* the pitch slot of utterance 2 without the round-up */
  if (host_gather(&s, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "store->pitch_off is not one ns_ds_plan wrote (entry 2 is 9, the plan's is 12)")) return 49;
  off[1][2] = saved;
  bs = s; bs.text_elems = 15;
  if (host_gather(&bs, &lens, order, 4, 1, &o) == 0 || !strstr(last_error(), "store->text is stated shorter")) return 50;
  for (i = 0; i < 3 * 7 * NMEL; ++i) if (mels[i] == mels[i]) return 51; /* a refused call writes nothing: still the NaN bytes */
  /* the device entry points: every refusal comes before the first HIP call */
  if (gather(&s, &lens, 0, order, 4, 1, &o, 0) == 0 || !strstr(last_error(), "null argument")) return 60;
  if (gather(&s, &lens, (const int32_t*)((char*)dev + 2), order, 4, 1, &o, 0) == 0 || !strstr(last_error(), "order_dev must be 4-byte aligned")) return 61;
  bo = o; bo.Tmax = 5;
  if (gather(&s, &lens, (const int32_t*)dev, order, 4, 1, &bo, 0) == 0 || !strstr(last_error(), "Tmax = 5 is below")) return 62;
  if (gather(&s, &lens, (const int32_t*)dev, order, 4, 2, &o, 0) == 0 || !strstr(last_error(), "first + B must not pass")) return 63;
  bo = o; bo.B = 1; bo.Tmax = 1 << 29;
  if (gather(&s, &lens, (const int32_t*)dev, order, 4, 0, &bo, 0) == 0 || !strstr(last_error(), "every output must stay below 2^31 elements")) return 64;
  if (op_gather(&s, &lens, (const int32_t*)dev, order, 4, 1, &o, 0, 0) == 0 || !strstr(last_error(), "grid_cap must lie in [1, 2048]")) return 65;
  if (op_gather(&s, &lens, (const int32_t*)dev, order, 4, 1, &o, NS_DS_GRID_CAP + 1, 0) == 0 || !strstr(last_error(), "grid_cap must lie in")) return 66;
  if (launches() != 0) return 67; /* a refused call launched nothing */
  /* the gather itself */
  if (host_gather(&s, &lens, order, 4, 1, &o) != 0) { printf("host gather: %s\n", last_error()); return 70; }
  for (b = 0; b < 3; ++b) {
    i = order[1 + b];
    if (small[b] != speaker[i] || small[3 + b] != text_len[i] || small[6 + b] != mel_len[i]) return 71;
    for (t = 0; t < 7; ++t) {
      for (c = 0; c < NMEL; ++c)
        if (mels[(b * 7 + t) * NMEL + c] != (t < mel_len[i] ? (float)(100 * i + t + 1000 * c) : 0.f)) return 72;
      if (energies[b * 7 + t] != (t < mel_len[i] ? (float)(100 * i + t) + 0.25f : 0.f)) return 73;
    }
    for (t = 0; t < 6; ++t) {
      if (pitches[b * 6 + t] != (t < text_len[i] ? (float)(100 * i + t) + 0.5f : 0.f)) return 74;
      if (texts[b * 6 + t] != (t < text_len[i] ? 100 * i + t + 1 : 0)) return 75;
    }
  }
  printf("batch of utterances 0, 2, 1 gathered on the host\n");
  printf("C caller ok\n");
  free(mel); free(pitch); free(energy); free(text); free(mels); free(pitches); free(energies); free(texts);
  return 0;
}
