// launch1d.h — the block size of the one-lane-per-item kernels and the grid that covers n items
// with it, for the units that launch such kernels (rollout.hip, noise.hip, ppo_batch.hip,
// ppo_loss.hip).  Not for the mlp units: they define block sizes of their own.
#pragma once
#include <hip/hip_runtime.h>

namespace {
constexpr int TPB = 256;
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + TPB - 1) / TPB)); }
}  // namespace
