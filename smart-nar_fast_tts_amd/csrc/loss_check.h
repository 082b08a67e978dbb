// The argument checks the loss's C-ABI families share (loss_api.hip defines them; lossgrad_api.hip uses them too): one statement of
// what a well-formed ns_loss_args is.  Host-side only; nothing here calls HIP.
#pragma once
#include "../../include/nar_fs2.h"
#include "host_core.h"

namespace ns {
// sizes, strides, null and misaligned pointers of the tensors the shape makes non-empty; reports as "<who>: ..." and fills `out`
int loss_check_args(const ns_loss_args* a, const char* who, LossArgs* out);
// the partial-slot workspace and the seven outputs
int loss_check_ws(const ns_loss_args* a, const void* ws, size_t ws_bytes, const float* out7, const char* who);
}  // namespace ns
