// Host build of the view's shared helpers (csrc/hg_view_shapes.h: every function there is __host__
// __device__).  TEST INFRASTRUCTURE ONLY: tests/test_view_cases.py compiles this file into a shared
// object, loads it with ctypes and runs the intersections and the shading on the CPU against
// tests/view_ref.py.  Nothing here launches a kernel.
#include "hg_view_shapes.h"

// ray[k] = (ox, oy, oz, dx, dy, dz, far); row: one world-table row (16 floats) per ray, already in
// the ray's coordinates (rel = 0).  out[k] = (hit, t, nx, ny, nz)
extern "C" void view_ray_rows_host(int n, const float* ray, const float* rows, float* out) {
  for (int k = 0; k < n; k++) {
    const float* r = ray + 7 * (size_t)k;
    float t = -1.f;
    hv3 nn = hv_mk(0.f, 0.f, 0.f);
    const bool hit = hv_ray_row(rows + 16 * (size_t)k, hv_mk(0.f, 0.f, 0.f), hv_mk(r[0], r[1], r[2]), hv_mk(r[3], r[4], r[5]),
                                r[6], &t, &nn);
    float* o = out + 5 * (size_t)k;
    o[0] = hit ? 1.f : 0.f; o[1] = t; o[2] = nn.x; o[3] = nn.y; o[4] = nn.z;
  }
}

// the nearest of ns rows for one ray given the terrain's t: returns the index or -1
extern "C" int view_nearest_host(const float* ray, const float* rows, int ns, float tmax, float* t) {
  hv3 nn;
  return hv_nearest_shape(rows, ns, hv_mk(0.f, 0.f, 0.f), hv_mk(ray[0], ray[1], ray[2]), hv_mk(ray[3], ray[4], ray[5]), tmax,
                          t, &nn);
}

// in[k] = (cls, hx, hy, nx, ny, nz, dx, dy, dz) as doubles; rgb[k][3]
extern "C" void view_shade_host(int n, const double* in, uint8_t* rgb) {
  for (int k = 0; k < n; k++) {
    const double* v = in + 9 * (size_t)k;
    hv_shade((int)v[0], v[1], v[2], hv_mk((float)v[3], (float)v[4], (float)v[5]), hv_mk((float)v[6], (float)v[7], (float)v[8]),
             rgb + 3 * (size_t)k);
  }
}

// the shape table of a model: out[s] = (kind, body, a[3], b[3], r) as floats; returns the count
extern "C" int view_table_host(const hg_model* m, float* out) {
  HvTable T;
  hv_build_table(m, &T);
  for (int s = 0; s < T.n; s++) {
    float* o = out + 9 * (size_t)s;
    o[0] = (float)T.s[s].kind; o[1] = (float)T.s[s].body;
    for (int i = 0; i < 3; i++) { o[2 + i] = T.s[s].a[i]; o[5 + i] = T.s[s].b[i]; }
    o[8] = T.s[s].r;
  }
  return T.n;
}
