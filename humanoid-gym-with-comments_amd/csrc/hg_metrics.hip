// hg_metrics.hip — gait metrics on the device (hg_metrics_sample / hg_metrics_fold, include/hgsim.h):
// per-env float64 accumulators of command tracking, distance, mechanical work, tilt, foot slip,
// support phases and peak torque, sampled on the physical pre-reset state between hg_step and
// hg_post and folded into per-env completed-episode rows after it.
//
// One thread per env, coalesced reads of the SoA arena, no LDS, no atomics, no cross-env reduction:
// every thread owns column e of the three metrics buffers, so the launches are order-independent
// and capturable.  Rows e >= n of the padded arena are never written.  The per-env arithmetic is
// hg_metrics_sample.h's (shared with the CPU tests).
#include "hg_common.h"
#include "hg_metrics_sample.h"

namespace {

constexpr int MET_T = 256;

__global__ __launch_bounds__(MET_T) void k_metrics_sample(HgState S, HgMetrics M, double dt) {
  const int e = blockIdx.x * MET_T + threadIdx.x;
  if (e >= S.n) return;
  const hg_cfg* c = S.cfg;
  const HgMetricsIn in = {S.root, S.commands, S.torques, S.dof_vel, S.contact, S.rigid, S.actions, S.last_actions};
  hg_metrics_sample_env(in, S.np, e, c->feet_body, c->torque_limit, dt, M.run, M.count);
}

// mode 0: the envs whose reset_buf the latest post launch set and whose running row holds a sample
// end their episode; mode 1: the masked envs' (mask NULL: all) running rows are discarded
__global__ __launch_bounds__(MET_T) void k_metrics_fold(HgState S, HgMetrics M, int mode,
                                                        const uint8_t* __restrict__ mask) {
  const int e = blockIdx.x * MET_T + threadIdx.x;
  if (e >= S.n) return;
  const size_t np = (size_t)S.np;
  double* run = M.run + e;
  if (mode == 1) {
    if (mask != nullptr && mask[e] == 0) return;
    for (int k = 0; k < HG_METRICS_SLOTS; k++) run[k * np] = 0.0;
    return;
  }
  if (S.reset_buf[e] == 0 || !(run[0] > 0.0)) return;
  double* done = M.done + e;
  for (int k = 0; k < HG_METRICS_SLOTS - 1; k++) {
    done[k * np] += run[k * np];
    run[k * np] = 0.0;
  }
  const int pk = HG_METRICS_SLOTS - 1;
  done[pk * np] = run[pk * np] > done[pk * np] ? run[pk * np] : done[pk * np];
  run[pk * np] = 0.0;
  M.count[0 * np + e] += 1;
  M.count[(S.time_out[e] == 0 ? 1 : 2) * np + e] += 1;
}

}  // namespace

extern "C" int hg_launch_metrics_sample(const HgState* S, const HgMetrics* M, double dt, hipStream_t stream) {
  hipLaunchKernelGGL(k_metrics_sample, dim3((S->n + MET_T - 1) / MET_T), dim3(MET_T), 0, stream, *S, *M, dt);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

extern "C" int hg_launch_metrics_fold(const HgState* S, const HgMetrics* M, int mode, const uint8_t* mask,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(k_metrics_fold, dim3((S->n + MET_T - 1) / MET_T), dim3(MET_T), 0, stream, *S, *M, mode, mask);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
