// Schedules every optimiser kernel derives on the device from the count of successful steps (optim.hip's adamw_ema_kernel,
// cf_train.hip's lagrange_step_kernel): one statement each, so that a second optimiser cannot drift from the first.
#pragma once

namespace cgen {

// EMA (utils.py:169-193) seen by the step that follows `t0` successful ones: a negative value means a straight copy (calls that
// see step <= update_after, +1 for the first 'initted' call), else the decay min(1 - 1 / (1 + t0 - update_after), beta).
__device__ __forceinline__ float ema_decay_of(int t0, int update_after, float beta) {
  if (t0 > update_after + 1) {
    const float epoch = (float)(t0 - update_after);
    const float d = 1.f - 1.f / (1.f + epoch);
    return d < beta ? d : beta;
  }
  return -1.f;
}

}  // namespace cgen
