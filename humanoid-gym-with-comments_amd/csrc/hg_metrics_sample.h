// hg_metrics_sample.h — one env's gait-metrics sample (hg_metrics_sample, include/hgsim.h has the
// slot table).  __host__ __device__: k_metrics_sample (hg_metrics.hip) and the CPU tests' host shim
// (tests/metrics_host_shim.hip) run this very function.
//
// Every f32 input is converted to double (exact) and all arithmetic is double, in the order written
// here, with floating-point contraction off (no fused multiply-add), so a float64 restatement that
// keeps the order differs only by the rounding of sqrt and divide.  Sums run over joints 0..11 and
// over the two feet in index order.  Nothing is written unless every input read is finite.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define HG_METRICS_SLOTS 13
#define HG_METRICS_COUNTS 4  // episodes, falls, time_outs, skipped
#define HG_METRICS_CONTACT_Z 5.0  // a foot is in contact when its world contact force z is > 5 (strict)

// the SoA rows the sample reads, each with env stride 1 and row stride np (HgState's regions)
struct HgMetricsIn {
  const float* root;          // [13][np] pos3 quat(xyzw)4 linvel3 angvel3, world
  const float* commands;      // [4][np]
  const float* torques;       // [12][np]
  const float* dof_vel;       // [12][np]
  const float* contact;       // [13*3][np]
  const float* rigid;         // [13*13][np]
  const float* actions;       // [12][np]
  const float* last_actions;  // [12][np]
};

// v rotated by the inverse of the unit quaternion (x, y, z, w): torch_utils.quat_rotate_inverse's
// expression, a - b + c with a = v (2 w^2 - 1), b = 2 w (q_v x v), c = 2 (q_v . v) q_v
__host__ __device__ inline void hg_metrics_rotate_inverse(double x, double y, double z, double w, const double v[3],
                                                          double out[3]) {
#pragma clang fp contract(off)
  const double s = 2.0 * w * w - 1.0;
  const double cx = y * v[2] - z * v[1], cy = z * v[0] - x * v[2], cz = x * v[1] - y * v[0];
  const double d = 2.0 * (x * v[0] + y * v[1] + z * v[2]);
  const double w2 = w * 2.0;
  out[0] = v[0] * s - w2 * cx + d * x;
  out[1] = v[1] * s - w2 * cy + d * y;
  out[2] = v[2] * s - w2 * cz + d * z;
}

// Adds env e's sample to run[slot * np + e] (slot 12: running max) — or, when any input read is
// non-finite, leaves the row alone and increments count[3 * np + e] (skipped).  Inputs read: root
// rows 3..12, commands rows 0..2, all 12 rows of torques / dof_vel / actions / last_actions, the
// contact-force z and the world linear velocity x, y (rigid fields 7, 8) of bodies feet[0], feet[1].
// dt: the policy step, (double)sim_dt * decimation.  Returns 1 when the sample was added.
__host__ __device__ inline int hg_metrics_sample_env(const HgMetricsIn& in, int np, int e, const int32_t feet[2],
                                                     const float torque_limit[12], double dt, double* run,
                                                     int32_t* count) {
#pragma clang fp contract(off)
  const size_t st = (size_t)np;
  bool bad = false;
  auto ld = [&](const float* p, int row) {
    const double v = (double)p[(size_t)row * st + e];
    bad |= !(v - v == 0.0);
    return v;
  };
  double q[4], vw[3], ww[3], c[3], tau[12], qd[12], a[12], ap[12], fz[2], fv[2][2];
  for (int i = 0; i < 4; i++) q[i] = ld(in.root, 3 + i);
  for (int i = 0; i < 3; i++) vw[i] = ld(in.root, 7 + i);
  for (int i = 0; i < 3; i++) ww[i] = ld(in.root, 10 + i);
  for (int i = 0; i < 3; i++) c[i] = ld(in.commands, i);
  for (int j = 0; j < 12; j++) {
    tau[j] = ld(in.torques, j);
    qd[j] = ld(in.dof_vel, j);
    a[j] = ld(in.actions, j);
    ap[j] = ld(in.last_actions, j);
  }
  for (int f = 0; f < 2; f++) {
    fz[f] = ld(in.contact, feet[f] * 3 + 2);
    fv[f][0] = ld(in.rigid, feet[f] * 13 + 7);
    fv[f][1] = ld(in.rigid, feet[f] * 13 + 8);
  }
  if (bad) {
    count[3 * st + e] += 1;
    return 0;
  }
  // the root quaternion normalised as k_depth does: one reciprocal of the norm, four products
  const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double qx = q[0] * qn, qy = q[1] * qn, qz = q[2] * qn, qw = q[3] * qn;
  const double grav[3] = {0.0, 0.0, -1.0};
  double vb[3], wb[3], gb[3];
  hg_metrics_rotate_inverse(qx, qy, qz, qw, vw, vb);
  hg_metrics_rotate_inverse(qx, qy, qz, qw, ww, wb);
  hg_metrics_rotate_inverse(qx, qy, qz, qw, grav, gb);
  const double ex = vb[0] - c[0], ey = vb[1] - c[1], ez = wb[2] - c[2];
  double work = 0.0, tq2 = 0.0, ar2 = 0.0, peak = 0.0;
  for (int j = 0; j < 12; j++) {
    const double p = tau[j] * qd[j];
    work += p > 0.0 ? p : 0.0;  // the clamp is per joint: negative power is not credited
    tq2 += tau[j] * tau[j];
    const double da = a[j] - ap[j];
    ar2 += da * da;
    const double r = fabs(tau[j]) / (double)torque_limit[j];
    peak = r > peak ? r : peak;
  }
  double slip = 0.0;
  int touching = 0;
  for (int f = 0; f < 2; f++) {
    if (fz[f] > HG_METRICS_CONTACT_Z) {
      slip += sqrt(fv[f][0] * fv[f][0] + fv[f][1] * fv[f][1]);
      touching++;
    }
  }
  double* r = run + e;
  r[0 * st] += 1.0;
  r[1 * st] += ex * ex;
  r[2 * st] += ey * ey;
  r[3 * st] += ez * ez;
  r[4 * st] += sqrt(vw[0] * vw[0] + vw[1] * vw[1]) * dt;
  r[5 * st] += work * dt;
  r[6 * st] += tq2 * dt;
  r[7 * st] += gb[0] * gb[0] + gb[1] * gb[1];
  r[8 * st] += slip * dt;
  r[9 * st] += ar2;
  r[10 * st] += touching == 2 ? 1.0 : 0.0;
  r[11 * st] += touching == 0 ? 1.0 : 0.0;
  r[12 * st] = peak > r[12 * st] ? peak : r[12 * st];
  return 1;
}
