// hg_depth.hip — the base-mounted depth camera (hg_render_depth, include/hgsim.h): one ray per
// pixel, marched through the triangulated heightfield K_step's contact code stands on (ground(),
// hg_physics.hip: cells split along the (i,j)-(i+1,j+1) diagonal), so the image shows exactly the
// surface the robot collides with.
//
// Formulation (no ray-triangle tests).  Along a ray o + t D the gap g(t) = z(t) - h(x(t), y(t)) is
// continuous and piecewise linear; its breakpoints are the ray's crossings of the grid lines x = i,
// y = j and of a cell diagonal u = v.  The kernel walks those segments in t order — a 2-D DDA over
// cells, each cell cut once more where the ray crosses its diagonal — evaluates g at the segment
// ends with ground()'s expression and returns the linear root of the first segment whose end
// values differ in sign or touch zero.  Neighbouring segments share their end point, and the sign
// the previous segment ended with is carried into the next one, so rounding between two cells'
// expressions cannot open a crack; the sign test is symmetric, which is the two-sided rule.
//
// Precision: the ray origin's grid coordinates are formed in float64 once per thread (positions
// reach 200 m, where a float32 ulp is 15 um) and split into an integer cell and a fraction; all
// per-segment arithmetic then runs in float32 in coordinates relative to that cell.
//
// Bounds: the march runs over the t-interval in which the ray lies inside the field's extent and
// inside [0, far], so every cell it loads is inside the field; the loop's trip count is fixed at
// launch (hg_launch_depth), the cell is re-checked before every load, and a non-finite pose,
// pitch or direction writes far_clip without entering the loop.
#include <math.h>

#include "hg_common.h"

namespace {

struct DepthParams {
  int W, H;
  float inv_fx;              // 1 / fx, fx = (W / 2) / tan(fov / 2)
  float half_w, half_h;      // W / 2, H / 2
  float pos[3];
  float near_clip, far_clip;
  int normalize;
  float noise;
  int max_steps;             // trip bound of the cell loop
  int tiles_x, tiles;        // 8 x 8 pixel tiles per row / per image (tile mapping)
  int64_t env_stride;
  uint64_t counter;
};

constexpr int DEPTH_T = 256;  // 4 waves

// ground()'s height inside one cell: lower triangle (u >= v) or upper
__host__ __device__ __forceinline__ float cell_h(bool lower, float u, float v, float h00, float h10, float h01, float h11) {
  u = fminf(fmaxf(u, 0.f), 1.f);
  v = fminf(fmaxf(v, 0.f), 1.f);
  return lower ? h00 + u * (h10 - h00) + v * (h11 - h10) : h00 + v * (h01 - h00) + u * (h11 - h01);
}

// +1 / -1 / 0 (0 also for NaN)
__host__ __device__ __forceinline__ int sgn(float x) { return (x > 0.f) - (x < 0.f); }

// Planar depth t in [0, zfar] of the ray (px + offx, py + offy, oz) + t (Dx, Dy, Dz) against the
// scene (field: the heightfield hf [rows][C]; else the plane z = 0), zfar when nothing is hit.
// __host__ too: the march can be run on a CPU against the tests' reference without a device.
__host__ __device__ inline float depth_march(bool field, const int16_t* __restrict__ hf, int rows, int C, float hs,
                                             float vs, float border, float px, float py, float offx, float offy,
                                             float oz, float Dx, float Dy, float Dz, float zfar, int max_steps) {
  float t = zfar;  // no hit
  const float chk = px + py + oz + offx + offy + Dx + Dy + Dz;
  if (chk - chk == 0.f) {  // every input finite
    if (!field) {
      // the plane z = 0, either side
      const float th = -oz / Dz;
      if (Dz != 0.f && th >= 0.f && th <= zfar) t = th;
      else if (oz == 0.f) t = 0.f;
    } else {
      // origin in grid units: integer cell + fraction, in float64
      const double gx = ((double)px + (double)offx + (double)border) / (double)hs;
      const double gy = ((double)py + (double)offy + (double)border) / (double)hs;
      if (fabs(gx) < 1e6 && fabs(gy) < 1e6) {
        const double fi = floor(gx), fj = floor(gy);
        const int i0 = (int)fi, j0 = (int)fj;
        const float u0 = (float)(gx - fi), v0 = (float)(gy - fj);
        const float dgx = Dx / hs, dgy = Dy / hs;
        const float ix = 1.0f / dgx, iy = 1.0f / dgy;  // inf on an axis-parallel ray: never used then
        // the t-interval inside the extent [0, rows - 1] x [0, cols - 1] and [0, zfar]
        float t0 = 0.f, t1 = zfar;
        const float lox = (float)(-i0), hix = (float)(rows - 1 - i0), loy = (float)(-j0), hiy = (float)(C - 1 - j0);
        if (dgx != 0.f) {
          const float a = (lox - u0) * ix, b = (hix - u0) * ix;
          t0 = fmaxf(t0, fminf(a, b));
          t1 = fminf(t1, fmaxf(a, b));
        } else if (u0 < lox || u0 > hix) {
          t1 = -1.f;
        }
        if (dgy != 0.f) {
          const float a = (loy - v0) * iy, b = (hiy - v0) * iy;
          t0 = fmaxf(t0, fminf(a, b));
          t1 = fminf(t1, fmaxf(a, b));
        } else if (v0 < loy || v0 > hiy) {
          t1 = -1.f;
        }
        if (t0 <= t1) {
          int ci = (int)floorf(fmaf(t0, dgx, u0)), cj = (int)floorf(fmaf(t0, dgy, v0));
          const int sx = dgx > 0.f ? 1 : -1, sy = dgy > 0.f ? 1 : -1;
          // the surface's boundary is closed: a ray that starts on u == rows - 1 (v == cols - 1) and does
          // not move inward is in the last cell at u = 1 (v = 1), as in ground(); one moving inward gets
          // there by the zero-length first segment
          const bool ei = dgx >= 0.f && i0 + ci == rows - 1, ej = dgy >= 0.f && j0 + cj == C - 1;
          ci -= ei;
          cj -= ej;
          float ts = t0;
          int prev = 0;  // sign g ended the previous segment with (0: none)
          const float ddiag = dgx - dgy, idiag = 1.0f / ddiag;  // idiag unused when ddiag == 0
          for (int k = 0; k < max_steps; k++) {
            // where the ray leaves this cell
            const float tx = dgx != 0.f ? ((float)(ci + (sx > 0)) - u0) * ix : INFINITY;
            const float ty = dgy != 0.f ? ((float)(cj + (sy > 0)) - v0) * iy : INFINITY;
            const float te = fmaxf(fminf(fminf(tx, ty), t1), ts);
            const int ai = i0 + ci, aj = j0 + cj;
            if (ai >= 0 && ai <= rows - 2 && aj >= 0 && aj <= C - 2) {
              const int16_t* p = hf + (size_t)ai * C + aj;
              const float h00 = vs * p[0], h01 = vs * p[1], h10 = vs * p[C], h11 = vs * p[C + 1];
              const float fci = (float)ci, fcj = (float)cj;
              // the diagonal u = v cuts the cell's stretch of the ray at td (at most once)
              float td = ((v0 - fcj) - (u0 - fci)) * idiag;
              const bool cut = ddiag != 0.f && td > ts && td < te;
              td = cut ? td : te;
              const float tm = 0.5f * (ts + td);
              const bool lower = fmaf(tm, dgx, u0) - fci >= fmaf(tm, dgy, v0) - fcj;
              const float us = fmaf(ts, dgx, u0) - fci, vsn = fmaf(ts, dgy, v0) - fcj;
              const float ud = fmaf(td, dgx, u0) - fci, vd = fmaf(td, dgy, v0) - fcj;
              const float gs = fmaf(ts, Dz, oz) - cell_h(lower, us, vsn, h00, h10, h01, h11);
              const float gd = fmaf(td, Dz, oz) - cell_h(lower, ud, vd, h00, h10, h01, h11);
              if (prev * sgn(gs) < 0) { t = ts; break; }  // the sign flipped between two cells' expressions
              if ((gs >= 0.f && gd <= 0.f) || (gs <= 0.f && gd >= 0.f)) {
                t = gs == gd ? ts : ts + (td - ts) * (gs / (gs - gd));
                break;
              }
              prev = sgn(gd);
              if (cut) {
                const float ue = fmaf(te, dgx, u0) - fci, ve = fmaf(te, dgy, v0) - fcj;
                const float g2 = fmaf(td, Dz, oz) - cell_h(!lower, ud, vd, h00, h10, h01, h11);
                const float ge = fmaf(te, Dz, oz) - cell_h(!lower, ue, ve, h00, h10, h01, h11);
                if (prev * sgn(g2) < 0) { t = td; break; }
                if ((g2 >= 0.f && ge <= 0.f) || (g2 <= 0.f && ge >= 0.f)) {
                  t = g2 == ge ? td : td + (te - td) * (g2 / (g2 - ge));
                  break;
                }
                prev = sgn(ge);
              }
            } else {
              prev = 0;  // no surface outside the field: nothing to carry
            }
            if (!(te < t1)) break;
            if (tx <= ty) ci += sx;
            if (ty <= tx) cj += sy;
            ts = te;
          }
          t = fminf(fmaxf(t, 0.f), zfar);
        }
      }
    }
  }
  return t;
}

// The launch parameters of a camera; shared with hg_depth_robot.hip.  The arguments were checked.
inline DepthParams depth_params(const hg_cfg* hcfg, const hg_depth_cam* cam, int64_t env_stride, uint64_t counter) {
  DepthParams P;
  P.W = cam->width;
  P.H = cam->height;
  const double half_fov = 0.5 * (double)cam->horizontal_fov_deg * (M_PI / 180.0);
  const double tan_h = tan(half_fov);
  P.inv_fx = (float)(tan_h / (0.5 * P.W));
  P.half_w = 0.5f * P.W;
  P.half_h = 0.5f * P.H;
  for (int i = 0; i < 3; i++) P.pos[i] = cam->pos[i];
  P.near_clip = cam->near_clip;
  P.far_clip = cam->far_clip;
  P.normalize = cam->normalize != 0;
  P.noise = cam->noise;
  // trip bound: a ray of planar depth far is far |d| long, |d| <= dmax at the image corner, and a
  // segment of L cells' length crosses at most sqrt(2) L + 2 cells; never more than the field has
  // rows + columns (the march stays inside the extent)
  P.max_steps = 1;
  if (hcfg->terrain_type != 0 && hcfg->heightfield != nullptr) {
    const double dmax = sqrt(1.0 + tan_h * tan_h * (1.0 + ((double)P.H / P.W) * ((double)P.H / P.W)));
    const double geo = ceil((double)cam->far_clip * dmax / (double)hcfg->hf_horizontal_scale * 1.4142135623730951) + 4.0;
    const double ext = (double)hcfg->hf_rows + (double)hcfg->hf_cols + 4.0;
    P.max_steps = (int)(geo < ext ? geo : ext);  // geo is NaN-free: the arguments are finite
    if (P.max_steps < 1) P.max_steps = 1;
  }
  P.tiles_x = (P.W + 7) / 8;
  P.tiles = P.tiles_x * ((P.H + 7) / 8);
  P.env_stride = env_stride;
  P.counter = counter;
  return P;
}

// The pixel's value from its planar depth t: noise, clamp, normalisation (include/hgsim.h).
__device__ __forceinline__ float depth_pixel_value(const hg_cfg* cfg, const DepthParams& P, int e, int pix, float t) {
  float d = t;
  if (P.noise > 0.f) {
    const u4 w = rng4(cfg, (uint32_t)e, P.counter, (uint32_t)pix >> 2, RNG_DEPTH_NOISE);
    const int k = pix & 3;
    const uint32_t word = k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w));
    d += P.noise * (2.0f * u01(word) - 1.0f);
  }
  d = fminf(fmaxf(d, P.near_clip), P.far_clip);
  if (P.normalize) d = (d - P.near_clip) / (P.far_clip - P.near_clip) - 0.5f;
  return d;
}

#ifndef HG_DEPTH_MARCH_ONLY  // hg_view.hip and hg_depth_robot.hip include this file for the march and the helpers alone
// TILE: a wave is an 8 x 8 pixel tile (its 64 rays walk the same few cells); else 64 consecutive
// pixels of the row-major image.
template <bool TILE>
__global__ __launch_bounds__(DEPTH_T, 8) void k_depth(HgState S, DepthParams P, const float* __restrict__ pitch,
                                                   float* __restrict__ out) {
  const hg_cfg* cfg = S.cfg;
  int r, c;
  if (TILE) {
    const int tile = blockIdx.x * (DEPTH_T / 64) + (threadIdx.x >> 6);
    if (tile >= P.tiles) return;
    const int l = threadIdx.x & 63;
    r = (tile / P.tiles_x) * 8 + (l >> 3);
    c = (tile % P.tiles_x) * 8 + (l & 7);
    if (r >= P.H || c >= P.W) return;
  } else {
    const int pix = blockIdx.x * DEPTH_T + threadIdx.x;
    if (pix >= P.W * P.H) return;
    r = pix / P.W;
    c = pix - r * P.W;
  }
  const int pix = r * P.W + c;
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
    const float t = depth_march(field, hf, rows, C, hs, vs, border, px, py, off.x, off.y, oz, D.x, D.y, D.z, zfar,
                                P.max_steps);
    out[(size_t)e * P.env_stride + pix] = depth_pixel_value(cfg, P, e, pix, t);
  }
}

#endif

}  // namespace

#ifndef HG_DEPTH_MARCH_ONLY
// mapping: 0 = 8 x 8 pixel tile per wave, 1 = 64 consecutive row-major pixels per wave.  The
// arguments were checked by hg_render_depth.
extern "C" int hg_launch_depth(const HgState* S, const hg_cfg* hcfg, const hg_depth_cam* cam, const float* pitch,
                               float* out, int64_t env_stride, uint64_t counter, int mapping, hipStream_t stream) {
  const DepthParams P = depth_params(hcfg, cam, env_stride, counter);
  const unsigned gy = (unsigned)(S->n < 65535 ? S->n : 65535);
  if (mapping == 0) {
    const unsigned gx = (unsigned)((P.tiles + DEPTH_T / 64 - 1) / (DEPTH_T / 64));
    hipLaunchKernelGGL(k_depth<true>, dim3(gx, gy), dim3(DEPTH_T), 0, stream, *S, P, pitch, out);
  } else {
    const unsigned gx = (unsigned)((P.W * P.H + DEPTH_T - 1) / DEPTH_T);
    hipLaunchKernelGGL(k_depth<false>, dim3(gx, gy), dim3(DEPTH_T), 0, stream, *S, P, pitch, out);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
#endif
