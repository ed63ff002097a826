// hg_depth_robot.h — the camera-relative shape rows of hg_render_depth_robot (include/hgsim.h) and
// the pixel rectangle that lets the pixel kernel skip a shape for a whole 8 x 8 tile.
// __host__ __device__: hg_depth_robot.hip runs it on the GPU, tests/depth_robot_host_shim.hip on
// the CPU.
//
// CAMERA-RELATIVE ROW (16 floats, the layout of hg_view_shapes.h's world row): positions are
// relative to the CAMERA ORIGIN o = p_base + R_base pos, in world axes, so the pixel kernel's ray
// origin is 0 and nothing the size of a capsule is ever added to a 200 m root position.  The slots
// a world row leaves 0 hold the shape's pixel rectangle, as floats:
//   [11] r0, [12] r1, [13] c0, [14] c1: rows r0 .. r1 and columns c0 .. c1, inclusive; the empty
//   rectangle is written as (0, -1, 0, -1), whose r1 lies above every tile, so the tile test of
//   k_depth_robot skips it in every tile, the first included.
//
// RECTANGLE (conservative: every pixel one of whose rays can hit the shape lies inside).  The shape's
// bounding sphere (capsule: the segment's midpoint, half its length + r; box: the centre, |half
// extents|; the radius padded by 1e-4 relative + 1e-5 m against float32 rounding) is taken to the
// camera frame (x forward, y left, z up: the world axes fwd / left / up of R_base R_y(pitch)).  A
// pixel's ray is (1, dy, dz) t in that frame with t >= 0, so it only reaches points with x = t >= 0:
//   - x_c + rho < 0 (wholly behind the camera plane): empty;
//   - x_c - rho <= 0 (touches or crosses the plane; an origin inside the shape is such a case), or
//     any non-finite value: the whole image;
//   - else dy = y / x and dz = z / x are bounded over the sphere's axis-aligned box, mapped to
//     columns c + 0.5 = W/2 - dy fx and rows r + 0.5 = H/2 - dz fx, and rounded outward by a pixel
//     (floor - 1, ceil + 1), which also covers sub-pixel sample offsets far above the +-0.01 the tests use.
#pragma once
#include "hg_view_shapes.h"

#define HD_RECT 11  // first rectangle slot of a row

// lo .. hi of the ratio v / x for v in [vl, vh], x in [xl, xh], 0 < xl
__host__ __device__ __forceinline__ void hd_ratio_bounds(float vl, float vh, float xl, float xh, float* lo, float* hi) {
  *hi = vh > 0.f ? vh / xl : vh / xh;
  *lo = vl < 0.f ? vl / xl : vl / xh;
}

// rect[0..3] = r0, r1, c0, c1 of a row under the camera axes fwd / left / up, fx in pixels
__host__ __device__ inline void hd_pixel_rect(const float* row, hv3 fwd, hv3 left, hv3 up, float fx, int W, int H,
                                              float rect[4]) {
  const int kind = (int)row[0];
  hv3 c = hv_mk(row[1], row[2], row[3]);
  float rho;
  if (kind == HV_CAPSULE) {
    const hv3 h = hv_mul(0.5f, hv_sub(hv_mk(row[4], row[5], row[6]), c));
    c = hv_add(c, h);
    rho = sqrtf(hv_dot(h, h)) + row[7];
  } else {
    rho = sqrtf(row[4] * row[4] + row[5] * row[5] + row[6] * row[6]);
  }
  rho = rho * 1.0001f + 1e-5f;
  const float x = hv_dot(fwd, c), y = hv_dot(left, c), z = hv_dot(up, c);
  rect[0] = 0.f; rect[1] = (float)(H - 1); rect[2] = 0.f; rect[3] = (float)(W - 1);  // the whole image
  if (!hv_finite(x + y + z + rho + fx)) return;
  if (x + rho < 0.f) {
    rect[0] = 0.f; rect[1] = -1.f; rect[2] = 0.f; rect[3] = -1.f;
    return;
  }
  if (x - rho <= 0.f) return;
  float ylo, yhi, zlo, zhi;
  hd_ratio_bounds(y - rho, y + rho, x - rho, x + rho, &ylo, &yhi);
  hd_ratio_bounds(z - rho, z + rho, x - rho, x + rho, &zlo, &zhi);
  // clamped before rounding: x - rho may be tiny and the ratios huge
  const float c0 = floorf(fminf(fmaxf(0.5f * W - yhi * fx - 0.5f, -2.f), (float)W + 2.f)) - 1.f;
  const float c1 = ceilf(fminf(fmaxf(0.5f * W - ylo * fx - 0.5f, -2.f), (float)W + 2.f)) + 1.f;
  const float r0 = floorf(fminf(fmaxf(0.5f * H - zhi * fx - 0.5f, -2.f), (float)H + 2.f)) - 1.f;
  const float r1 = ceilf(fminf(fmaxf(0.5f * H - zlo * fx - 0.5f, -2.f), (float)H + 2.f)) + 1.f;
  rect[0] = fmaxf(r0, 0.f); rect[1] = fminf(r1, (float)(H - 1));
  rect[2] = fmaxf(c0, 0.f); rect[3] = fminf(c1, (float)(W - 1));
  if (rect[0] > rect[1] || rect[2] > rect[3]) { rect[0] = 0.f; rect[1] = -1.f; rect[2] = 0.f; rect[3] = -1.f; }
}
