// hg_depth_robot.hip — the base depth camera with the robot's own legs in view
// (hg_render_depth_robot, include/hgsim.h): hg_render_depth's image, every pixel the nearest of the
// terrain and the robot's drawn shapes.  Two kernels on the step path for ALL envs, no LDS, no
// atomics, no host synchronisation.
//
// Drawn shapes: the rows of hv_build_table (hg_view_shapes.h) whose body is not body 0 — for XBot-L
// the six leg capsules and the two foot boxes.  The camera is rigidly fixed to body 0, so that
// body's shapes (the base box, which contains the default camera position, and the hand capsules)
// never move in the image and are not drawn.
//
// k_depth_pose: one thread per (drawn shape, env), env fastest, so a wave walks one body's chain
// (hv_body_pose, hg_view_pose.h: the chain walk k_view_pose uses).  It writes the row relative to
// the camera origin in world axes, and the row's pixel rectangle under this env's camera
// (hg_depth_robot.h), into the arena's view_table region (16 rows of 16 floats per env; in-stream
// ordering with hg_render_view, which rewrites the rows it reads, is enough).
//
// k_depth_robot: k_depth's tile mapping, env loop, march and post-processing (hg_depth.hip).  After
// the march the env's rows are read as wave-uniform values; a row whose rectangle misses the wave's
// 8 x 8 tile is skipped in a uniform branch (most tiles see no shape), the others are intersected
// analytically (hv_ray_row) from the origin 0 with tmax = the best t so far, so a shape wins a tie
// with the terrain.  HG_DEPTH_MAP=rows is not supported here: the mapping is always tiles.
#include <math.h>

#define HG_DEPTH_MARCH_ONLY
#include "hg_depth.hip"
#include "hg_depth_robot.h"
#include "hg_view_pose.h"

namespace {

__global__ __launch_bounds__(DEPTH_T) void k_depth_pose(HgState S, HvTable T, DepthParams P,
                                                       const float* __restrict__ pitch, float* __restrict__ table) {
  const int idx = blockIdx.x * DEPTH_T + threadIdx.x;
  if (idx >= S.n * T.n) return;
  const int sh = idx / S.n, e = idx - sh * S.n;
  const int np = S.np;
  const HvLocal L = T.s[sh];
  float R[9];
  const hv3 ob = hv_body_pose(S, e, L.body, R);  // relative to the base origin
  // the camera: its origin relative to the base origin and its axes, as k_depth_robot forms them
  float qx = S.root[3 * np + e], qy = S.root[4 * np + e], qz = S.root[5 * np + e], qw = S.root[6 * np + e];
  const float qn = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
  qx *= qn; qy *= qn; qz *= qn; qw *= qn;
  float sp = 0.f, cp = 1.f;
  if (pitch) sincosf(pitch[e], &sp, &cp);
  const f3 oc = quat_apply(qx, qy, qz, qw, mk(P.pos[0], P.pos[1], P.pos[2]));
  const f3 fwd = quat_apply(qx, qy, qz, qw, mk(cp, 0.f, -sp));
  const f3 left = quat_apply(qx, qy, qz, qw, mk(0.f, 1.f, 0.f));
  const f3 up = quat_apply(qx, qy, qz, qw, mk(sp, 0.f, cp));
  const hv3 o = hv_sub(ob, hv_mk(oc.x, oc.y, oc.z));
  float v[HV_ROW];
#pragma unroll
  for (int i = 0; i < HV_ROW; i++) v[i] = 0.f;
  const hv3 a = hv_add(o, mat3_vec(R, hv_mk(L.a[0], L.a[1], L.a[2])));
  v[0] = (float)L.kind;
  v[1] = a.x; v[2] = a.y; v[3] = a.z;
  if (L.kind == HV_CAPSULE) {
    const hv3 b = hv_add(o, mat3_vec(R, hv_mk(L.b[0], L.b[1], L.b[2])));
    v[4] = b.x; v[5] = b.y; v[6] = b.z;
    v[7] = L.r;
  } else {
    v[4] = L.b[0]; v[5] = L.b[1]; v[6] = L.b[2];
    mat_to_quat(R, v + 7);
  }
  hd_pixel_rect(v, hv_mk(fwd.x, fwd.y, fwd.z), hv_mk(left.x, left.y, left.z), hv_mk(up.x, up.y, up.z), 1.0f / P.inv_fx,
                P.W, P.H, v + HD_RECT);
  float4* row = (float4*)(table + ((size_t)e * HV_MAX_SHAPES + sh) * HV_ROW);
#pragma unroll
  for (int i = 0; i < HV_ROW / 4; i++) row[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

__global__ __launch_bounds__(DEPTH_T, 8) void k_depth_robot(HgState S, DepthParams P, const float* __restrict__ pitch,
                                                         const float* __restrict__ table, int ns,
                                                         float* __restrict__ out) {
  const hg_cfg* cfg = S.cfg;
  const int tile = blockIdx.x * (DEPTH_T / 64) + (threadIdx.x >> 6);
  if (tile >= P.tiles) return;
  const int l = threadIdx.x & 63;
  const int r = (tile / P.tiles_x) * 8 + (l >> 3);
  const int c = (tile % P.tiles_x) * 8 + (l & 7);
  if (r >= P.H || c >= P.W) return;
  const int pix = r * P.W + c;
  // the wave's tile as scalars: the rectangle tests below are uniform branches
  const int tile_u = __builtin_amdgcn_readfirstlane(tile);
  const float tr0 = (float)((tile_u / P.tiles_x) * 8), tc0 = (float)((tile_u % P.tiles_x) * 8);
  const bool field = cfg->terrain_type != 0 && cfg->heightfield != nullptr;
  const int16_t* __restrict__ hf = cfg->heightfield;
  const int rows = cfg->hf_rows, C = cfg->hf_cols;
  const float hs = cfg->hf_horizontal_scale, vs = cfg->hf_vertical_scale, border = cfg->hf_border;
  const float zfar = P.far_clip;

  for (int e = blockIdx.y; e < S.n; e += gridDim.y) {  // block-uniform env
    const int np = S.np;
    const float px = S.root[0 * np + e], py = S.root[1 * np + e], pz = S.root[2 * np + e];
    float qx = S.root[3 * np + e], qy = S.root[4 * np + e], qz = S.root[5 * np + e], qw = S.root[6 * np + e];
    const float qn = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
    qx *= qn; qy *= qn; qz *= qn; qw *= qn;
    float sp = 0.f, cp = 1.f;
    if (pitch) sincosf(pitch[e], &sp, &cp);
    // camera-frame direction, pitched about y (positive pitch: x turns toward -z), then the base rotation
    const float dcy = -((float)c + 0.5f - P.half_w) * P.inv_fx;
    const float dcz = -((float)r + 0.5f - P.half_h) * P.inv_fx;
    const f3 D = quat_apply(qx, qy, qz, qw, mk(cp + sp * dcz, dcy, cp * dcz - sp));
    const f3 off = quat_apply(qx, qy, qz, qw, mk(P.pos[0], P.pos[1], P.pos[2]));
    const float oz = pz + off.z;
    float t = depth_march(field, hf, rows, C, hs, vs, border, px, py, off.x, off.y, oz, D.x, D.y, D.z, zfar,
                          P.max_steps);
    // The shapes read a copy of D the optimiser cannot see through: everything up to here then has
    // k_depth's users, and this compiler gives it k_depth's arithmetic (the same packed and fused
    // operations), so the terrain's t is k_depth's bit for bit.  Nothing guarantees that by
    // construction — the two kernels are compiled apart, and another compiler version may pack or
    // fuse them differently — so tests/test_gpu_depth_robot.py::test_post_processing_is_shared holds
    // every image of the scene set to it.
    float sx = D.x, sy = D.y, sz = D.z;
    asm volatile("" : "+v"(sx), "+v"(sy), "+v"(sz));
    const hv3 Ds = hv_mk(sx, sy, sz);
    const float* __restrict__ rowsp = table + (size_t)e * HV_MAX_SHAPES * HV_ROW;
    for (int k = 0; k < ns; k++) {
      const float* __restrict__ row = rowsp + (size_t)k * HV_ROW;
      if (row[HD_RECT + 1] < tr0 || row[HD_RECT] > tr0 + 7.f || row[HD_RECT + 3] < tc0 || row[HD_RECT + 2] > tc0 + 7.f)
        continue;
      float tk;
      hv3 nk;
      if (hv_ray_row(row, hv_mk(0.f, 0.f, 0.f), hv_mk(0.f, 0.f, 0.f), Ds, t, &tk, &nk)) t = tk;
    }
    out[(size_t)e * P.env_stride + pix] = depth_pixel_value(cfg, P, e, pix, t);
  }
}

}  // namespace

// The arguments were checked by hg_render_depth_robot (hg_api.hip); table: the arena's view_table
// region, HV_MAX_SHAPES rows per env.
extern "C" int hg_launch_depth_robot(const HgState* S, const hg_cfg* hcfg, const hg_model* model, const hg_depth_cam* cam,
                                     const float* pitch, float* table, float* out, int64_t env_stride, uint64_t counter,
                                     hipStream_t stream) {
  const DepthParams P = depth_params(hcfg, cam, env_stride, counter);
  // the drawn shapes: the table's rows that are not on body 0
  HvTable all, T;
  hv_build_table(model, &all);
  T.n = 0;
  for (int s = 0; s < all.n; s++)
    if (all.s[s].body != 0) T.s[T.n++] = all.s[s];
  if (T.n > 0) {
    const unsigned gp = (unsigned)(((int64_t)S->n * T.n + DEPTH_T - 1) / DEPTH_T);
    hipLaunchKernelGGL(k_depth_pose, dim3(gp), dim3(DEPTH_T), 0, stream, *S, T, P, pitch, table);
  }
  const unsigned gx = (unsigned)((P.tiles + DEPTH_T / 64 - 1) / (DEPTH_T / 64));
  const unsigned gy = (unsigned)(S->n < 65535 ? S->n : 65535);
  hipLaunchKernelGGL(k_depth_robot, dim3(gx, gy), dim3(DEPTH_T), 0, stream, *S, P, pitch, table, T.n, out);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
