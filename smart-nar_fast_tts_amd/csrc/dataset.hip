// Training-batch gather for gfx950: the reference's collated, padded batch of B utterances out of the packed
// device-resident store in ONE launch.
//   k_ds_gather   every element of mels [B, Tmax, n_mel], pitches [B, Pmax], energies [B, Emax], texts [B, Lmax] (int64) and
//                 speakers / src_lens / mel_lens [B] (int64) for the utterances order[0 .. B): the store's bits below an utterance's
//                 length, +0.0 / 0 behind it.
// Geometry: the outputs are one flat list of work items (dataset.h): a thread takes one item a turn — a 16-byte group of a mel row
// (one 16-byte load, one 16-byte store; consecutive threads take consecutive groups, and a padded row's source is contiguous too)
// or one dword of the 1-D outputs, which are 1/80 of the bytes — and a workgroup of 256 threads takes the items blockIdx.x * 256 + t,
// then strides by the grid (capped by the launcher).  No LDS, no atomics, no workspace; control flow depends on the item index and on
// the length tables alone; nothing is read at or past the store's stated sizes.
#include "dataset.h"

namespace ns {

__global__ __launch_bounds__(DS_BLOCK) void k_ds_gather(const DsArgs a) {
  const int64_t step = (int64_t)gridDim.x * DS_BLOCK;
  int64_t w = (int64_t)blockIdx.x * DS_BLOCK + threadIdx.x;
  for (; w < a.w_mel; w += step) ds_mel_item(a, (uint32_t)w);
  for (; w < a.w_total; w += step) ds_tail_item(a, w);  // (a thread goes on where its stride left the mel range)
}

hipError_t launch_ds_gather(const DsArgs& a, int grid_cap, hipStream_t st) {
  if (a.w_total < 1 || grid_cap < 1 || grid_cap > DS_GRID_CAP) return hipErrorInvalidValue;
  const int64_t most = (a.w_total + DS_BLOCK - 1) / DS_BLOCK;
  hipLaunchKernelGGL(k_ds_gather, dim3((unsigned)(most < (int64_t)grid_cap ? most : (int64_t)grid_cap)), dim3(DS_BLOCK), 0, st, a);
  return hipGetLastError();
}

}  // namespace ns
