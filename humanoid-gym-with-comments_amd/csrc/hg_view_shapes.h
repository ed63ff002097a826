// hg_view_shapes.h — the robot's shape table, ray/shape intersections and the shading of the
// follow-camera view (hg_render_view, hg_view_shapes; include/hgsim.h).  Everything here is
// __host__ __device__: hg_view.hip runs it on the GPU, tests/view_host_shim.hip on the CPU.
//
// SHAPE TABLE (derived from hg_model alone; at most HV_MAX_SHAPES = 16 shapes, 11 for XBot-L), in
// this order:
//   1. every capsule with capsule_kind == 0 (thighs, shins, ankle rolls, hands), in capsule order:
//      segment capsule_p0..capsule_p1, capsule_radius, on capsule_body;
//   2. one FOOT BOX per body that owns foot-sole candidates (the first num_foot_contacts contacts),
//      in order of first appearance: the body-frame axis-aligned box bounding that body's sole points
//      and the body origin.  BUILD-DEFINED visual fit (the foot is not a collision box; K_step
//      collides the sole points);
//   3. the BASE BOX: the body-frame bounding box of the radius-0 contact candidates on body 0 (the
//      eight base-box corners).
// Arms above the wrist, neck and head are not collision shapes and are NOT drawn: the picture is a
// box on legs.
//
// WORLD TABLE ROW (16 floats per shape):
//   [0] kind: 0 capsule, 1 foot box, 2 base box
//   capsule: [1..3] world p0, [4..6] world p1, [7] radius
//   box:     [1..3] world centre, [4..6] half extents, [7..10] body rotation, xyzw quaternion
//   the rest 0.
//
// RAY RULES (ray o + t d, t in [0, far]; d need not be unit, t is in units of d):
//   - capsule: the cylinder quadratic between the end planes plus the two cap spheres, the
//     smallest entry t; p0 == p1 is a sphere.  Box: slabs in the box frame.
//   - an origin inside a shape (or on its surface) gives t = 0 with that shape; the normal of such a
//     hit is -d / |d|.
//   - a hit exactly at far counts; a shape wholly behind the origin is a miss.
//   - any non-finite input (origin, direction, shape) gives a miss.
//   - among shapes the nearest t wins and ties go to the lower index; a tie between terrain and a
//     shape goes to the shape (hv_nearest_shape is told the terrain's t and only has to beat or
//     equal it).
//   - terrain is two-sided, as in depth_march; a terrain t equal to far is "nothing hit" (sky).
//
// SHADING CONSTANTS (hv_shade; tests restate them from here):
//   light L = normalize(0.3, 0.2, 0.9); ambient 0.35, diffuse 0.65
//   colour = round(255 * clamp(albedo * (0.35 + 0.65 * max(0, n . L)), 0, 1)), n flipped to face the ray
//   terrain: 1 m world-xy checker, (0.55, 0.55, 0.50) where floor(x) + floor(y) is even,
//            (0.40, 0.40, 0.36) where odd; its normal is the hit triangle's plane
//   capsules (0.85, 0.45, 0.15); foot boxes (0.20, 0.20, 0.20); base box (0.25, 0.35, 0.70)
//   sky (0.53, 0.71, 0.92), unshaded
// IDS: 0 sky, 1 terrain, 2 + k shape k of the table.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hgsim.h"

#define HV_MAX_SHAPES 16
#define HV_ROW 16
#define HV_CAPSULE 0
#define HV_FOOT_BOX 1
#define HV_BASE_BOX 2
#define HV_ID_SKY 0
#define HV_ID_TERRAIN 1
#define HV_ID_SHAPE0 2

struct hv3 { float x, y, z; };
__host__ __device__ __forceinline__ hv3 hv_mk(float x, float y, float z) { return {x, y, z}; }
__host__ __device__ __forceinline__ hv3 hv_add(hv3 a, hv3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__host__ __device__ __forceinline__ hv3 hv_sub(hv3 a, hv3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ hv3 hv_mul(float s, hv3 a) { return {s * a.x, s * a.y, s * a.z}; }
__host__ __device__ __forceinline__ float hv_dot(hv3 a, hv3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ __forceinline__ hv3 hv_cross(hv3 a, hv3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// rotate v by the unit xyzw quaternion q (inv: by its inverse)
__host__ __device__ __forceinline__ hv3 hv_rot(const float q[4], hv3 v, bool inv) {
  const hv3 u = inv ? hv_mk(-q[0], -q[1], -q[2]) : hv_mk(q[0], q[1], q[2]);
  const hv3 t = hv_mul(2.0f, hv_cross(u, v));
  return hv_add(hv_add(v, hv_mul(q[3], t)), hv_cross(u, t));
}
__host__ __device__ __forceinline__ bool hv_finite(float s) { return s - s == 0.f; }

// one shape in its body's frame: a capsule's p0 / p1 / r, or a box's centre / half extents
struct HvLocal {
  int32_t kind, body;
  float a[3], b[3], r;
};
struct HvTable {
  int32_t n;
  HvLocal s[HV_MAX_SHAPES];
};

// the shape table of a model (see SHAPE TABLE above)
inline void hv_build_table(const hg_model* m, HvTable* T) {
  T->n = 0;
  for (int k = 0; k < m->num_capsules && T->n < HV_MAX_SHAPES; k++) {
    if (m->capsule_kind[k] != 0) continue;
    HvLocal& s = T->s[T->n++];
    s.kind = HV_CAPSULE;
    s.body = m->capsule_body[k];
    for (int i = 0; i < 3; i++) { s.a[i] = m->capsule_p0[k][i]; s.b[i] = m->capsule_p1[k][i]; }
    s.r = m->capsule_radius[k];
  }
  // pass 0: the foot boxes (bodies of the sole candidates, the origin included); pass 1: the base box
  for (int pass = 0; pass < 2; pass++) {
    int seen[HG_MAX_CONTACTS], nseen = 0;
    const int c0 = 0, c1 = pass == 0 ? m->num_foot_contacts : m->num_contacts;
    for (int c = c0; c < c1; c++) {
      const int body = m->contact_body[c];
      if (pass == 1 && (body != 0 || m->contact_radius[c] != 0.f || c < m->num_foot_contacts)) continue;
      bool dup = false;
      for (int i = 0; i < nseen; i++) dup = dup || seen[i] == body;
      if (dup || T->n >= HV_MAX_SHAPES) continue;
      seen[nseen++] = body;
      float lo[3], hi[3];
      bool first = true;
      if (pass == 0) { for (int i = 0; i < 3; i++) lo[i] = hi[i] = 0.f; first = false; }
      for (int d = c; d < c1; d++) {
        if (m->contact_body[d] != body) continue;
        if (pass == 1 && (m->contact_radius[d] != 0.f || d < m->num_foot_contacts)) continue;
        for (int i = 0; i < 3; i++) {
          const float v = m->contact_pos[d][i];
          lo[i] = first ? v : fminf(lo[i], v);
          hi[i] = first ? v : fmaxf(hi[i], v);
        }
        first = false;
      }
      HvLocal& s = T->s[T->n++];
      s.kind = pass == 0 ? HV_FOOT_BOX : HV_BASE_BOX;
      s.body = body;
      for (int i = 0; i < 3; i++) { s.a[i] = 0.5f * (lo[i] + hi[i]); s.b[i] = 0.5f * (hi[i] - lo[i]); }
      s.r = 0.f;
    }
  }
}

// entry of the ray into the sphere |x - c| = r, oc = o - c; the origin is known to be outside
__host__ __device__ __forceinline__ bool hv_sphere_entry(hv3 oc, hv3 d, float dd, float r, float* t) {
  // move the origin to the point of the ray nearest the centre: the quadratic is then b = 0
  const float tm = -hv_dot(oc, d) / dd;
  const hv3 m = hv_add(oc, hv_mul(tm, d));
  const float h = r * r - hv_dot(m, m);
  if (!(h >= 0.f)) return false;
  *t = tm - sqrtf(h / dd);
  return true;
}

// Ray / capsule.  true: *t in [0, far] and the unit outward normal *n (-d / |d| at t = 0).
__host__ __device__ inline bool hv_ray_capsule(hv3 o, hv3 d, hv3 p0, hv3 p1, float r, float far, float* t, hv3* n) {
  const float chk = o.x + o.y + o.z + d.x + d.y + d.z + p0.x + p0.y + p0.z + p1.x + p1.y + p1.z + r + far;
  const float dd = hv_dot(d, d);
  if (!hv_finite(chk) || !(dd > 0.f) || !(r >= 0.f)) return false;
  const hv3 ba = hv_sub(p1, p0), oa = hv_sub(o, p0);
  const float baba = hv_dot(ba, ba);
  // origin inside: its distance to the segment is at most r
  const float s0 = baba > 0.f ? fminf(fmaxf(hv_dot(oa, ba) / baba, 0.f), 1.f) : 0.f;
  const hv3 w0 = hv_sub(oa, hv_mul(s0, ba));
  const float inv_d = 1.0f / sqrtf(dd);
  if (hv_dot(w0, w0) <= r * r) {
    *t = 0.f;
    *n = hv_mul(-inv_d, d);
    return true;
  }
  float best = INFINITY;
  hv3 bn = hv_mk(0.f, 0.f, 0.f);
  float ts;
  if (hv_sphere_entry(oa, d, dd, r, &ts) && ts >= 0.f) {
    best = ts;
    bn = hv_mul(1.0f / r, hv_add(oa, hv_mul(ts, d)));
  }
  if (baba > 0.f) {
    const hv3 ob = hv_sub(o, p1);
    if (hv_sphere_entry(ob, d, dd, r, &ts) && ts >= 0.f && ts < best) {
      best = ts;
      bn = hv_mul(1.0f / r, hv_add(ob, hv_mul(ts, d)));
    }
    // the cylinder about the unit axis u, from the point of the ray nearest the segment's midpoint
    // (keeps the quadratic's terms the size of the capsule, not of the camera distance)
    const hv3 u = hv_mul(1.0f / sqrtf(baba), ba);
    const hv3 om = hv_sub(oa, hv_mul(0.5f, ba));
    const float tm = -hv_dot(om, d) / dd;
    const hv3 m = hv_add(om, hv_mul(tm, d));  // relative to the midpoint
    const float du = hv_dot(d, u), mu = hv_dot(m, u);
    const float a = dd - du * du;
    const float b = hv_dot(m, d) - mu * du;
    const float c = hv_dot(m, m) - mu * mu - r * r;
    const float h = b * b - a * c;
    if (a > 0.f && h >= 0.f) {
      const float tc = tm + (-b - sqrtf(h)) / a;
      const float y = mu + (tc - tm) * du;  // along the axis, from the midpoint
      const float half = 0.5f * sqrtf(baba);
      if (tc >= 0.f && tc < best && fabsf(y) <= half) {
        best = tc;
        const hv3 p = hv_add(m, hv_mul(tc - tm, d));
        bn = hv_mul(1.0f / r, hv_sub(p, hv_mul(y, u)));
      }
    }
  }
  if (!(best <= far)) return false;
  *t = best;
  *n = bn;
  return true;
}

// Ray / box (centre c, half extents h, rotation q xyzw).  As hv_ray_capsule.
__host__ __device__ inline bool hv_ray_box(hv3 o, hv3 d, hv3 c, hv3 h, const float q[4], float far, float* t, hv3* n) {
  const float chk = o.x + o.y + o.z + d.x + d.y + d.z + c.x + c.y + c.z + h.x + h.y + h.z + q[0] + q[1] + q[2] + q[3] + far;
  const float dd = hv_dot(d, d);
  if (!hv_finite(chk) || !(dd > 0.f)) return false;
  const hv3 ol = hv_rot(q, hv_sub(o, c), true), dl = hv_rot(q, d, true);
  const float oo[3] = {ol.x, ol.y, ol.z}, dv[3] = {dl.x, dl.y, dl.z}, hh[3] = {h.x, h.y, h.z};
  float tn = -INFINITY, tf = INFINITY;
  int axis = 0;
  for (int i = 0; i < 3; i++) {
    if (dv[i] != 0.f) {
      const float inv = 1.0f / dv[i];
      const float t1 = (-hh[i] - oo[i]) * inv, t2 = (hh[i] - oo[i]) * inv;
      const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
      if (lo > tn) { tn = lo; axis = i; }
      tf = fminf(tf, hi);
    } else if (fabsf(oo[i]) > hh[i]) {
      return false;
    }
  }
  if (!(tn <= tf) || tf < 0.f) return false;
  if (tn <= 0.f) {  // origin inside or on the surface
    *t = 0.f;
    *n = hv_mul(-1.0f / sqrtf(dd), d);
    return true;
  }
  if (!(tn <= far)) return false;
  *t = tn;
  const float sg = dv[axis] > 0.f ? -1.f : 1.f;
  *n = hv_rot(q, hv_mk(axis == 0 ? sg : 0.f, axis == 1 ? sg : 0.f, axis == 2 ? sg : 0.f), false);
  return true;
}

// One world-table row against a ray; rel is subtracted from the row's positions first (the caller's
// local origin, so that 200 m world coordinates do not eat the mantissa; o is relative to it too).
__host__ __device__ inline bool hv_ray_row(const float* row, hv3 rel, hv3 o, hv3 d, float far, float* t, hv3* n) {
  const int kind = (int)row[0];
  const hv3 a = hv_sub(hv_mk(row[1], row[2], row[3]), rel);
  if (kind == HV_CAPSULE) {
    const hv3 b = hv_sub(hv_mk(row[4], row[5], row[6]), rel);
    return hv_ray_capsule(o, d, a, b, row[7], far, t, n);
  }
  if (kind == HV_FOOT_BOX || kind == HV_BASE_BOX) return hv_ray_box(o, d, a, hv_mk(row[4], row[5], row[6]), row + 7, far, t, n);
  return false;
}

// The nearest shape of `ns` rows that hits at t <= tmax (the terrain's t, or far): its index or -1.
__host__ __device__ inline int hv_nearest_shape(const float* rows, int ns, hv3 rel, hv3 o, hv3 d, float tmax, float* t,
                                                hv3* n) {
  int best = -1;
  float bt = tmax;
  for (int k = 0; k < ns; k++) {
    float tk;
    hv3 nk;
    if (hv_ray_row(rows + (size_t)k * HV_ROW, rel, o, d, tmax, &tk, &nk) && (best < 0 ? tk <= bt : tk < bt)) {
      best = k;
      bt = tk;
      *n = nk;
    }
  }
  if (best >= 0) *t = bt;
  return best;
}

// Colour class of a hit: 0 sky, 1 terrain, 2 capsule, 3 foot box, 4 base box.
__host__ __device__ __forceinline__ int hv_class(int id, int kind) { return id < HV_ID_SHAPE0 ? id : 2 + kind; }

// The pixel's colour (see SHADING CONSTANTS): cls from hv_class, (hx, hy) the hit point's world xy
// (terrain checker only), n the unit normal (either orientation), d the ray direction.
__host__ __device__ inline void hv_shade(int cls, double hx, double hy, hv3 n, hv3 d, uint8_t rgb[3]) {
  float al[3] = {0.53f, 0.71f, 0.92f};
  float k = 1.0f;
  if (cls != 0) {
    if (cls == 1) {
      const long long par = (long long)floor(hx) + (long long)floor(hy);
      if (par & 1) { al[0] = 0.40f; al[1] = 0.40f; al[2] = 0.36f; }
      else { al[0] = 0.55f; al[1] = 0.55f; al[2] = 0.50f; }
    } else if (cls == 2) { al[0] = 0.85f; al[1] = 0.45f; al[2] = 0.15f; }
    else if (cls == 3) { al[0] = 0.20f; al[1] = 0.20f; al[2] = 0.20f; }
    else { al[0] = 0.25f; al[1] = 0.35f; al[2] = 0.70f; }
    if (hv_dot(n, d) > 0.f) n = hv_mul(-1.0f, n);
    const float il = 1.0f / sqrtf(0.3f * 0.3f + 0.2f * 0.2f + 0.9f * 0.9f);
    const float nl = (0.3f * n.x + 0.2f * n.y + 0.9f * n.z) * il;
    k = 0.35f + 0.65f * fmaxf(0.f, nl);
  }
  for (int i = 0; i < 3; i++) {
    const float v = fminf(fmaxf(al[i] * k, 0.f), 1.f);
    rgb[i] = (uint8_t)rintf(255.0f * v);
  }
}
