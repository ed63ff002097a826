// hg_view.hip — the follow-camera view of robot and terrain (hg_view_shapes, hg_render_view;
// include/hgsim.h): what play.py records.  Two kernels, no LDS, no host synchronisation.
//
// k_view_pose: forward kinematics of the selected envs from root_states and dof_pos through
// hg_model's parent / joint_pos / joint_rot / axis — NOT from HG_T_RIGID_STATE, which only K_step
// writes and which therefore still holds the old pose after a masked reset or a write through the
// views.  One thread per (env, shape) walks its body's chain from the base down, relative to the
// base origin; the root position is added last, so a robot 200 m from the origin keeps its
// mantissa.  Output: the world shape table (hg_view_shapes.h, 16 floats per shape).
//
// k_view: one ray per pixel, 8 x 8 pixel tiles per wave and envs on blockIdx.y, as k_depth.  The
// terrain's t comes from depth_march (hg_depth.hip, included as tests/depth_host_shim.hip includes
// it); every shape of the env's table — read as wave-uniform values — is intersected analytically
// (hg_view_shapes.h) in coordinates relative to the env's base position; the nearest t in [0, far]
// wins and the hit is shaded.  The march's trip bound is fixed at launch as in hg_launch_depth and
// the march itself never leaves the field's extent, wherever the camera is.
#include <math.h>

#define HG_DEPTH_MARCH_ONLY
#include "hg_depth.hip"
#include "hg_view_pose.h"
#include "hg_view_shapes.h"

namespace {

struct ViewParams {
  int W, H;
  float inv_fx, half_w, half_h;
  int mode;
  float eye[3];
  float fwd[3], left[3], up[3];  // camera axes in the world: x forward, y left, z up
  float far_clip;
  int max_steps;
  int tiles_x, tiles;
  int n, ns;                     // selected envs, shapes per env
};

constexpr int VIEW_T = 256;  // 4 waves

// the env a selected row renders, -1 when env_ids names none
__device__ __forceinline__ int view_env(const HgState& S, const int32_t* env_ids, int k) {
  const int e = env_ids ? env_ids[k] : k;
  return (e >= 0 && e < S.n) ? e : -1;
}

__global__ __launch_bounds__(VIEW_T) void k_view_pose(HgState S, HvTable T, const int32_t* __restrict__ env_ids, int n,
                                                     float* __restrict__ out) {
  const int idx = blockIdx.x * VIEW_T + threadIdx.x;
  if (idx >= n * HV_MAX_SHAPES) return;
  const int k = idx / HV_MAX_SHAPES, sh = idx - k * HV_MAX_SHAPES;
  float* row = out + (size_t)idx * HV_ROW;
  float v[HV_ROW];
#pragma unroll
  for (int i = 0; i < HV_ROW; i++) v[i] = 0.f;
  const int e = view_env(S, env_ids, k);
  if (sh >= T.n || e < 0) {
    v[0] = -1.f;  // no shape
  } else {
    const HvLocal L = T.s[sh];
    const int np = S.np;
    float R[9];
    const hv3 o = hv_body_pose(S, e, L.body, R);  // relative to the base origin
    const hv3 root = hv_mk(S.root[0 * np + e], S.root[1 * np + e], S.root[2 * np + e]);
    const hv3 a = hv_add(hv_add(o, mat3_vec(R, hv_mk(L.a[0], L.a[1], L.a[2]))), root);
    v[0] = (float)L.kind;
    v[1] = a.x; v[2] = a.y; v[3] = a.z;
    if (L.kind == HV_CAPSULE) {
      const hv3 b = hv_add(hv_add(o, mat3_vec(R, hv_mk(L.b[0], L.b[1], L.b[2]))), root);
      v[4] = b.x; v[5] = b.y; v[6] = b.z;
      v[7] = L.r;
    } else {
      v[4] = L.b[0]; v[5] = L.b[1]; v[6] = L.b[2];
      mat_to_quat(R, v + 7);
    }
  }
#pragma unroll
  for (int i = 0; i < HV_ROW; i++) row[i] = v[i];
}

__global__ __launch_bounds__(VIEW_T) void k_view(HgState S, ViewParams P, const int32_t* __restrict__ env_ids,
                                                const float* __restrict__ table, uint8_t* __restrict__ rgb,
                                                float* __restrict__ depth, uint8_t* __restrict__ ids) {
  const hg_cfg* cfg = S.cfg;
  const int tile = blockIdx.x * (VIEW_T / 64) + (threadIdx.x >> 6);
  if (tile >= P.tiles) return;
  const int l = threadIdx.x & 63;
  const int r = (tile / P.tiles_x) * 8 + (l >> 3);
  const int c = (tile % P.tiles_x) * 8 + (l & 7);
  if (r >= P.H || c >= P.W) return;
  const int pix = r * P.W + c;
  const bool field = cfg->terrain_type != 0 && cfg->heightfield != nullptr;
  const int16_t* __restrict__ hf = cfg->heightfield;
  const int rows = cfg->hf_rows, C = cfg->hf_cols;
  const float hs = cfg->hf_horizontal_scale, vs = cfg->hf_vertical_scale, border = cfg->hf_border;
  const float zfar = P.far_clip;
  // the pixel's direction: t is the planar depth along the camera's x axis (fwd . D = 1)
  const float dcy = -((float)c + 0.5f - P.half_w) * P.inv_fx;
  const float dcz = -((float)r + 0.5f - P.half_h) * P.inv_fx;
  const hv3 D = hv_mk(P.fwd[0] + dcy * P.left[0] + dcz * P.up[0], P.fwd[1] + dcy * P.left[1] + dcz * P.up[1],
                      P.fwd[2] + dcy * P.left[2] + dcz * P.up[2]);

  for (int k = blockIdx.y; k < P.n; k += gridDim.y) {  // block-uniform selected env
    const int e = view_env(S, env_ids, k);
    const int np = S.np;
    const float nanv = __int_as_float(0x7fc00000);
    const float px = e >= 0 ? S.root[0 * np + e] : nanv, py = e >= 0 ? S.root[1 * np + e] : nanv;
    const float pz = e >= 0 ? S.root[2 * np + e] : nanv;
    // the local frame's origin is the base position; the eye relative to it
    // (a world camera still sees the terrain when the pose is not finite; the shapes then miss)
    const bool follow = P.mode == 1;
    const hv3 o = follow ? hv_mk(P.eye[0], P.eye[1], P.eye[2]) : hv_mk(P.eye[0] - px, P.eye[1] - py, P.eye[2] - pz);
    const float mx = follow ? px : 0.f, my = follow ? py : 0.f;  // depth_march adds them to the offset in float64
    const float ex = P.eye[0], ey = P.eye[1], ez = follow ? pz + P.eye[2] : P.eye[2];
    float t = depth_march(field, hf, rows, C, hs, vs, border, mx, my, ex, ey, ez, D.x, D.y, D.z, zfar, P.max_steps);
    int id = t < zfar ? HV_ID_TERRAIN : HV_ID_SKY;
    int kind = 0;
    hv3 nrm = hv_mk(0.f, 0.f, 1.f);
    const float* __restrict__ rowsp = table + (size_t)k * HV_MAX_SHAPES * HV_ROW;
    float ts;
    hv3 ns;
    const int hit = hv_nearest_shape(rowsp, P.ns, hv_mk(px, py, pz), o, D, t, &ts, &ns);
    if (hit >= 0) {
      id = HV_ID_SHAPE0 + hit;
      kind = (int)rowsp[(size_t)hit * HV_ROW];
      t = ts;
      nrm = ns;
    }
    const size_t at = (size_t)k * P.W * P.H + pix;
    if (depth) depth[at] = t;
    if (ids) ids[at] = (uint8_t)id;
    if (rgb) {
      double hx = 0.0, hy = 0.0;
      if (id == HV_ID_TERRAIN) {
        hx = ((double)mx + (double)ex) + (double)t * (double)D.x;
        hy = ((double)my + (double)ey) + (double)t * (double)D.y;
        if (field) {
          // the hit triangle's plane: ground()'s cell and split at the hit point
          const double gx = (hx + (double)border) / (double)hs, gy = (hy + (double)border) / (double)hs;
          int i = (int)floor(gx), j = (int)floor(gy);
          i = i < 0 ? 0 : (i > rows - 2 ? rows - 2 : i);
          j = j < 0 ? 0 : (j > C - 2 ? C - 2 : j);
          const float u = (float)(gx - (double)i), v = (float)(gy - (double)j);
          const int16_t* p = hf + (size_t)i * C + j;
          const float h00 = vs * p[0], h01 = vs * p[1], h10 = vs * p[C], h11 = vs * p[C + 1];
          const bool lower = u >= v;
          const float dx = (lower ? h10 - h00 : h11 - h01) / hs, dy = (lower ? h11 - h10 : h01 - h00) / hs;
          const float inv = 1.0f / sqrtf(dx * dx + dy * dy + 1.0f);
          nrm = hv_mk(-dx * inv, -dy * inv, inv);
        }
      }
      uint8_t col[3];
      hv_shade(hv_class(id, kind), hx, hy, nrm, D, col);
      uint8_t* q = rgb + 3 * at;
      q[0] = col[0]; q[1] = col[1]; q[2] = col[2];
    }
  }
}

}  // namespace

// The arguments were checked by hg_view_shapes / hg_render_view (hg_api.hip).
extern "C" int hg_launch_view_pose(const HgState* S, const hg_model* model, const int32_t* env_ids, int n, float* out,
                                   int* num_shapes, hipStream_t stream) {
  HvTable T;
  hv_build_table(model, &T);
  if (num_shapes) *num_shapes = T.n;
  const unsigned gx = (unsigned)(((int64_t)n * HV_MAX_SHAPES + VIEW_T - 1) / VIEW_T);
  hipLaunchKernelGGL(k_view_pose, dim3(gx), dim3(VIEW_T), 0, stream, *S, T, env_ids, n, out);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// fwd / left / up: the camera's unit axes in the world (hg_render_view computed them in float64).
extern "C" int hg_launch_view(const HgState* S, const hg_cfg* hcfg, const hg_view_cam* cam, const double* fwd,
                              const double* left, const double* up, const int32_t* env_ids, int n, int num_shapes,
                              const float* table, uint8_t* rgb, float* depth, uint8_t* ids, hipStream_t stream) {
  ViewParams P;
  P.W = cam->width;
  P.H = cam->height;
  const double tan_h = tan(0.5 * (double)cam->horizontal_fov_deg * (M_PI / 180.0));
  P.inv_fx = (float)(tan_h / (0.5 * P.W));
  P.half_w = 0.5f * P.W;
  P.half_h = 0.5f * P.H;
  P.mode = cam->mode;
  for (int i = 0; i < 3; i++) {
    P.eye[i] = cam->eye[i];
    P.fwd[i] = (float)fwd[i];
    P.left[i] = (float)left[i];
    P.up[i] = (float)up[i];
  }
  P.far_clip = cam->far_clip;
  // trip bound, as hg_launch_depth: a ray of planar depth far is far |d| long, |d| <= dmax at the
  // image corner; never more than the field has rows + columns (the march stays inside the extent)
  P.max_steps = 1;
  if (hcfg->terrain_type != 0 && hcfg->heightfield != nullptr) {
    const double dmax = sqrt(1.0 + tan_h * tan_h * (1.0 + ((double)P.H / P.W) * ((double)P.H / P.W)));
    const double geo = ceil((double)cam->far_clip * dmax / (double)hcfg->hf_horizontal_scale * 1.4142135623730951) + 4.0;
    const double ext = (double)hcfg->hf_rows + (double)hcfg->hf_cols + 4.0;
    P.max_steps = (int)(geo < ext ? geo : ext);
    if (P.max_steps < 1) P.max_steps = 1;
  }
  P.tiles_x = (P.W + 7) / 8;
  P.tiles = P.tiles_x * ((P.H + 7) / 8);
  P.n = n;
  P.ns = num_shapes;
  const unsigned gx = (unsigned)((P.tiles + VIEW_T / 64 - 1) / (VIEW_T / 64));
  const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
  hipLaunchKernelGGL(k_view, dim3(gx, gy), dim3(VIEW_T), 0, stream, *S, P, env_ids, table, rgb, depth, ids);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
