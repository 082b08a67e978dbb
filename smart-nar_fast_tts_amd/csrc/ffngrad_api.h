// What the two matmul modes of the ns_fg_* family share on the host side: ffngrad_api.hip (exact fp32) defines these, and
// ffngrad_bf16_api.hip (the opt-in "bf16" mode) checks its arguments with them, in the same words, and counts
// its launches into the same thread-local counter, so ns_fg_last_launches reports either mode's calls.  Host-only.
#pragma once
#include "../../include/nar_fs2.h"
#include "train_api.h"

namespace ns {
namespace fg {

int* launches();  // the calling thread's ns_fg_* launch counter
int check_dims(const ns_fg_shape& s, const std::string& w);
std::vector<NamedPtr> params(const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_g, const float* ln_b);
// the ReLU gate and, where d_b1 is wanted, the fixed-order sum of its partials: one or two launches, counted
int relu_gate(const float* da, const float* h, int M, int di, float* dh, float* d_b1, double* part, hipStream_t st);

}  // namespace fg
}  // namespace ns
