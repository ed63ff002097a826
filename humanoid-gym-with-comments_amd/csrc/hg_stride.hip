// hg_stride.hip — stride statistics on the device (hg_cfg.gait_metrics bit 1; hg_metrics_sample /
// hg_metrics_fold launch these next to k_metrics_*, include/hgsim.h): a per-env, per-foot detector of
// lift-off, apex and touchdown that accumulates swing time, foot clearance, step length and width,
// touchdown force, stride length and stride time in float64, sampled on the physical pre-reset state
// between hg_step and hg_post and folded into per-env completed rows after it.
//
// One thread per env owns both feet (step width needs the other foot), coalesced reads of the SoA
// arena, no LDS, no atomics, no cross-env reduction: every thread owns column e of the three stride
// buffers, so the launches are order-independent and capturable.  Columns e >= n of the padded arena
// are never written.  The per-env arithmetic is hg_stride_sample.h's (shared with the CPU tests).
#include "hg_common.h"
#include "hg_stride_sample.h"

namespace {

constexpr int STR_T = 256;

__global__ __launch_bounds__(STR_T) void k_stride_sample(HgState S, HgStride R, double dt) {
  const int e = blockIdx.x * STR_T + threadIdx.x;
  if (e >= S.n) return;
  const hg_cfg* c = S.cfg;
  const HgStrideIn in = {S.root, S.contact, S.rigid};
  hg_stride_sample_env(in, S.np, e, c->feet_body, c->heightfield, c->hf_rows, c->hf_cols, c->hf_horizontal_scale,
                       c->hf_vertical_scale, c->hf_border, c->terrain_type, dt, R.state, R.run);
}

// mode 0: the envs whose reset_buf the latest post launch set end their episode: the running rows are
// added to the completed ones and a swing in progress is discarded with the state; mode 1: the masked
// envs' (mask NULL: all) running rows and state are discarded
__global__ __launch_bounds__(STR_T) void k_stride_fold(HgState S, HgStride R, int mode,
                                                       const uint8_t* __restrict__ mask) {
  const int e = blockIdx.x * STR_T + threadIdx.x;
  if (e >= S.n) return;
  const size_t np = (size_t)S.np;
  if (mode == 1 ? (mask != nullptr && mask[e] == 0) : S.reset_buf[e] == 0) return;
  double* run = R.run + e;
  if (mode == 0) {
    double* done = R.done + e;
    for (int k = 0; k < 2 * HG_STRIDE_SLOTS; k++) done[k * np] += run[k * np];
  }
  for (int k = 0; k < 2 * HG_STRIDE_SLOTS; k++) run[k * np] = 0.0;
  double* state = R.state + e;
  for (int k = 0; k < 2 * HG_STRIDE_STATE_SLOTS; k++) state[k * np] = 0.0;
}

}  // namespace

extern "C" int hg_launch_stride_sample(const HgState* S, const HgStride* R, double dt, hipStream_t stream) {
  hipLaunchKernelGGL(k_stride_sample, dim3((S->n + STR_T - 1) / STR_T), dim3(STR_T), 0, stream, *S, *R, dt);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

extern "C" int hg_launch_stride_fold(const HgState* S, const HgStride* R, int mode, const uint8_t* mask,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(k_stride_fold, dim3((S->n + STR_T - 1) / STR_T), dim3(STR_T), 0, stream, *S, *R, mode, mask);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
