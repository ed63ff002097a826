// hg_stride_sample.h — one env's stride-detector sample (hg_metrics_sample with hg_cfg.gait_metrics
// bit 1, include/hgsim.h has the definitions and the slot tables).  __host__ __device__:
// k_stride_sample (hg_stride.hip) and the CPU tests' host shim (tests/stride_host_shim.hip) run this
// very function.
//
// Every f32 input is converted to double (exact) and all arithmetic is double, in the order written
// here, with floating-point contraction off (no fused multiply-add), so a float64 restatement that
// keeps the order differs only by the rounding of sqrt and divide.  Both feet's inputs are read
// first, then foot 0 is advanced, then foot 1.  Nothing is added unless every input read is finite.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hg_metrics_sample.h"  // HG_METRICS_CONTACT_Z: the same contact rule as the support fractions

#define HG_STRIDE_SLOTS 10        // accumulator slots per foot (HG_T_STRIDE_RUN / _DONE rows f * 10 + k)
#define HG_STRIDE_STATE_SLOTS 8   // state slots per foot (HG_T_STRIDE_STATE rows f * 8 + k)
#define HG_STRIDE_MIN_SWING 3     // a swing of fewer samples is contact chatter, not a step

// accumulator slots
enum {
  HG_SD_STRIDES = 0, HG_SD_SWING_TIME, HG_SD_CLEARANCE, HG_SD_STEP_LENGTH, HG_SD_STEP_WIDTH, HG_SD_TOUCHDOWN_FORCE,
  HG_SD_STRIDE_PAIRS, HG_SD_STRIDE_LENGTH, HG_SD_STRIDE_TIME, HG_SD_SHORT_SWINGS
};
// state slots; phase: 0 none, 1 stance, 2 swing, 3 swing whose lift-off was not seen
enum {
  HG_SS_PHASE = 0, HG_SS_PHASE_STEPS, HG_SS_SINCE_TD, HG_SS_HAS_ANCHOR, HG_SS_ANCHOR_X, HG_SS_ANCHOR_Y, HG_SS_REF_HAG,
  HG_SS_APEX_HAG
};

// the SoA rows the sample reads, each with env stride 1 and row stride np (HgState's regions)
struct HgStrideIn {
  const float* root;     // [13][np] pos3 quat(xyzw)4 linvel3 angvel3, world
  const float* contact;  // [13*3][np]
  const float* rigid;    // [13*13][np]
};

// Ground height under the world point (x, y), both finite: 0 on a plane (terrain_type 0 or no
// field); otherwise vertical_scale times the minimum of three neighbours of the cell
// (i, j) = ((p + border) / horizontal_scale, truncated, clipped to [0, rows-2] x [0, cols-2]):
// hg_terrain_sample's quantisation on the world point itself, no yaw rotation.  The measured-heights
// rule, not the triangulated surface: a foot next to a riser reads the lower tread.
__host__ __device__ inline double hg_stride_ground(const int16_t* hf, int rows, int cols, float hs, float vs,
                                                   float border, int terrain_type, double x, double y) {
#pragma clang fp contract(off)
  if (terrain_type == 0 || hf == nullptr) return 0.0;
  const double gi = trunc((x + (double)border) / (double)hs), gj = trunc((y + (double)border) / (double)hs);
  const double ri = (double)(rows - 2), cj = (double)(cols - 2);
  // the clip runs on the double, so no out-of-range value is ever converted to an integer
  const int i = (int)(!(gi >= 0.0) ? 0.0 : (gi > ri ? ri : gi));
  const int j = (int)(!(gj >= 0.0) ? 0.0 : (gj > cj ? cj : gj));
  int h = hf[(size_t)i * cols + j];
  const int h1 = hf[(size_t)(i + 1) * cols + j], h2 = hf[(size_t)i * cols + j + 1];
  h = h1 < h ? h1 : h;
  h = h2 < h ? h2 : h;
  return (double)vs * (double)h;
}

// Advances env e's two feet by one sample: state[(f * 8 + k) * np + e], run[(f * 10 + k) * np + e].
// Inputs read: root rows 3..6 (the quaternion), and of bodies feet[0], feet[1] the contact-force z and
// the world position x, y, z (rigid fields 0..2).  dt: the policy step, (double)sim_dt * decimation.
// When any of them is non-finite, or the heading's norm is not > 0, nothing is added and both feet's
// state rows are zeroed, so that no stride spans the gap.  Returns 1 when the sample was taken.
//
// clearance = apex_hag - ref_hag: the highest height above ground of the swing minus the height above
// ground of the last stance sample before lift-off.  It is negative when the foot only descends
// (stepping down a riser: the ground under the foot drops, then the foot follows).
__host__ __device__ inline int hg_stride_sample_env(const HgStrideIn& in, int np, int e, const int32_t feet[2],
                                                    const int16_t* hf, int rows, int cols, float hs, float vs,
                                                    float border, int terrain_type, double dt, double* state,
                                                    double* run) {
#pragma clang fp contract(off)
  const size_t st = (size_t)np;
  bool bad = false;
  auto ld = [&](const float* p, int row) {
    const double v = (double)p[(size_t)row * st + e];
    bad |= !(v - v == 0.0);
    return v;
  };
  double q[4], fz[2], p[2][3];
  for (int i = 0; i < 4; i++) q[i] = ld(in.root, 3 + i);
  for (int f = 0; f < 2; f++) {
    fz[f] = ld(in.contact, feet[f] * 3 + 2);
    for (int i = 0; i < 3; i++) p[f][i] = ld(in.rigid, feet[f] * 13 + i);
  }
  double hx = 0.0, hy = 0.0;
  if (!bad) {
    // the root quaternion normalised as hg_metrics_sample_env does: one reciprocal of the norm, four products
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double qx = q[0] * qn, qy = q[1] * qn, qz = q[2] * qn, qw = q[3] * qn;
    const double fx = 1.0 - 2.0 * (qy * qy + qz * qz), fy = 2.0 * (qx * qy + qz * qw);
    const double n = sqrt(fx * fx + fy * fy);
    if (n > 0.0) {
      hx = fx / n;
      hy = fy / n;
    } else {
      bad = true;  // a vertical base x axis (or a zero quaternion) has no heading
    }
  }
  double* s0 = state + e;
  if (bad) {
    for (int k = 0; k < 2 * HG_STRIDE_STATE_SLOTS; k++) s0[k * st] = 0.0;
    return 0;
  }
  double hag[2];
  for (int f = 0; f < 2; f++)
    hag[f] = p[f][2] - hg_stride_ground(hf, rows, cols, hs, vs, border, terrain_type, p[f][0], p[f][1]);
  for (int f = 0; f < 2; f++) {
    double* s = s0 + (size_t)(f * HG_STRIDE_STATE_SLOTS) * st;
    double* r = run + e + (size_t)(f * HG_STRIDE_SLOTS) * st;
    const bool contact = fz[f] > HG_METRICS_CONTACT_Z;
    const int phase = (int)s[HG_SS_PHASE * st];
    const double has_anchor = s[HG_SS_HAS_ANCHOR * st];
    if (phase == 0) {
      s[HG_SS_PHASE * st] = contact ? 1.0 : 3.0;
      s[HG_SS_PHASE_STEPS * st] = 1.0;
      s[(contact ? HG_SS_REF_HAG : HG_SS_APEX_HAG) * st] = hag[f];
    } else if (phase == 1) {
      s[HG_SS_SINCE_TD * st] += has_anchor;
      if (contact) {
        s[HG_SS_PHASE_STEPS * st] += 1.0;
        s[HG_SS_REF_HAG * st] = hag[f];
      } else {  // lift-off: ref_hag keeps the last stance sample
        s[HG_SS_PHASE * st] = 2.0;
        s[HG_SS_PHASE_STEPS * st] = 1.0;
        s[HG_SS_APEX_HAG * st] = hag[f];
      }
    } else if (!contact) {  // swing goes on
      s[HG_SS_SINCE_TD * st] += has_anchor;
      s[HG_SS_PHASE_STEPS * st] += 1.0;
      const double apex = s[HG_SS_APEX_HAG * st];
      s[HG_SS_APEX_HAG * st] = hag[f] > apex ? hag[f] : apex;
    } else {  // touchdown
      bool anchor_here = true;
      if (phase == 2) {
        const double since = s[HG_SS_SINCE_TD * st] + has_anchor;
        s[HG_SS_SINCE_TD * st] = since;
        const double steps = s[HG_SS_PHASE_STEPS * st];
        if (steps < (double)HG_STRIDE_MIN_SWING) {
          r[HG_SD_SHORT_SWINGS * st] += 1.0;  // chatter: the anchor and since_td are left alone
          anchor_here = false;
        } else {
          const double rx = p[f][0] - p[1 - f][0], ry = p[f][1] - p[1 - f][1];
          const double along = rx * hx + ry * hy, lat = ry * hx - rx * hy;
          r[HG_SD_STRIDES * st] += 1.0;
          r[HG_SD_SWING_TIME * st] += steps * dt;
          r[HG_SD_CLEARANCE * st] += s[HG_SS_APEX_HAG * st] - s[HG_SS_REF_HAG * st];
          r[HG_SD_STEP_LENGTH * st] += along;
          r[HG_SD_STEP_WIDTH * st] += fabs(lat);
          r[HG_SD_TOUCHDOWN_FORCE * st] += fz[f];
          if (has_anchor != 0.0) {
            const double dx = p[f][0] - s[HG_SS_ANCHOR_X * st], dy = p[f][1] - s[HG_SS_ANCHOR_Y * st];
            r[HG_SD_STRIDE_PAIRS * st] += 1.0;
            r[HG_SD_STRIDE_LENGTH * st] += sqrt(dx * dx + dy * dy);
            r[HG_SD_STRIDE_TIME * st] += since * dt;
          }
        }
      }
      if (anchor_here) {  // a valid swing, or a swing whose lift-off was not seen (no stride is counted)
        s[HG_SS_ANCHOR_X * st] = p[f][0];
        s[HG_SS_ANCHOR_Y * st] = p[f][1];
        s[HG_SS_HAS_ANCHOR * st] = 1.0;
        s[HG_SS_SINCE_TD * st] = 0.0;
      }
      s[HG_SS_PHASE * st] = 1.0;
      s[HG_SS_PHASE_STEPS * st] = 1.0;
      s[HG_SS_REF_HAG * st] = hag[f];
    }
  }
  return 1;
}
