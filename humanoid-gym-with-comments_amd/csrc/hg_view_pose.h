// hg_view_pose.h — forward kinematics of one body from root_states and dof_pos, shared by the two
// pose passes that draw the robot: k_view_pose (hg_view.hip, world rows for the follow-camera view)
// and k_depth_pose (hg_depth_robot.hip, camera-relative rows for the base depth camera).  Device
// only.  NOT from HG_T_RIGID_STATE, which only K_step writes and which therefore still holds the
// old pose after a masked reset or a write through the views.
#pragma once
#include "hg_common.h"
#include "hg_view_shapes.h"

__device__ __forceinline__ void mat3_mul(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ hv3 mat3_vec(const float* A, hv3 v) {
  return hv_mk(A[0] * v.x + A[1] * v.y + A[2] * v.z, A[3] * v.x + A[4] * v.y + A[5] * v.z, A[6] * v.x + A[7] * v.y + A[8] * v.z);
}
// rotation about the unit axis a by angle q (Rodrigues), row-major
__device__ __forceinline__ void axis_angle(hv3 a, float q, float* R) {
  float s, c;
  sincosf(q, &s, &c);
  const float k = 1.0f - c;
  R[0] = c + k * a.x * a.x;       R[1] = k * a.x * a.y - s * a.z; R[2] = k * a.x * a.z + s * a.y;
  R[3] = k * a.x * a.y + s * a.z; R[4] = c + k * a.y * a.y;       R[5] = k * a.y * a.z - s * a.x;
  R[6] = k * a.x * a.z - s * a.y; R[7] = k * a.y * a.z + s * a.x; R[8] = c + k * a.z * a.z;
}
// xyzw quaternion of a rotation matrix (the branch with the largest pivot), w >= 0 where it decides
__device__ __forceinline__ void mat_to_quat(const float* R, float* q) {
  const float tr = R[0] + R[4] + R[8];
  float x, y, z, w;
  if (tr > 0.f) {
    const float s = 2.0f * sqrtf(tr + 1.0f);
    w = 0.25f * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const float s = 2.0f * sqrtf(1.0f + R[0] - R[4] - R[8]);
    w = (R[7] - R[5]) / s; x = 0.25f * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const float s = 2.0f * sqrtf(1.0f + R[4] - R[0] - R[8]);
    w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25f * s; z = (R[5] + R[7]) / s;
  } else {
    const float s = 2.0f * sqrtf(1.0f + R[8] - R[0] - R[4]);
    w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25f * s;
  }
  const float inv = 1.0f / sqrtf(x * x + y * y + z * z + w * w);
  q[0] = x * inv; q[1] = y * inv; q[2] = z * inv; q[3] = w * inv;
}

// The pose of `body` of env e: walks the body's chain from the base down through hg_model's parent /
// joint_pos / joint_rot / axis.  R: the body's world rotation, row-major; the return value: its
// origin RELATIVE TO THE BASE ORIGIN in world axes (the caller adds the root position last, or not
// at all, so a robot 200 m from the origin keeps its mantissa).
__device__ inline hv3 hv_body_pose(const HgState& S, int e, int body, float* R) {
  const hg_model* __restrict__ M = S.model;
  const int np = S.np;
  // the body's chain, base first
  int chain[HG_MAX_BODIES], len = 0;
  for (int b = body; b > 0 && len < HG_MAX_BODIES; b = M->parent[b]) chain[len++] = b;
  float qx = S.root[3 * np + e], qy = S.root[4 * np + e], qz = S.root[5 * np + e], qw = S.root[6 * np + e];
  const float qn = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
  qx *= qn; qy *= qn; qz *= qn; qw *= qn;
  R[0] = 1.0f - 2.0f * (qy * qy + qz * qz); R[1] = 2.0f * (qx * qy - qz * qw); R[2] = 2.0f * (qx * qz + qy * qw);
  R[3] = 2.0f * (qx * qy + qz * qw); R[4] = 1.0f - 2.0f * (qx * qx + qz * qz); R[5] = 2.0f * (qy * qz - qx * qw);
  R[6] = 2.0f * (qx * qz - qy * qw); R[7] = 2.0f * (qy * qz + qx * qw); R[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
  hv3 o = hv_mk(0.f, 0.f, 0.f);
  for (int c = len - 1; c >= 0; c--) {
    const int b = chain[c];
    o = hv_add(o, mat3_vec(R, hv_mk(M->joint_pos[b][0], M->joint_pos[b][1], M->joint_pos[b][2])));
    float Rj[9], Rq[9];
    mat3_mul(R, M->joint_rot[b], Rj);
    axis_angle(hv_mk(M->axis[b][0], M->axis[b][1], M->axis[b][2]), S.dof_pos[(size_t)(b - 1) * np + e], Rq);
    mat3_mul(Rj, Rq, R);
  }
  return o;
}
