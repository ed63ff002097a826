// Host build of the depth camera's pixel rectangle (csrc/hg_depth_robot.h: hd_pixel_rect is
// __host__ __device__).  TEST INFRASTRUCTURE ONLY: tests/test_depth_robot_cases.py compiles this file
// into a shared object, loads it with ctypes and checks the rectangle on the CPU against the rays of
// tests/depth_ref.py and the intersections of tests/view_ref.py.  Nothing here launches a kernel.
#include "hg_depth_robot.h"

// rows[k]: one camera-relative row (16 floats); axes[k] = (fwd, left, up), 9 floats, the camera's
// axes in the world; rect[k] = (r0, r1, c0, c1)
extern "C" void depth_robot_rect_host(int n, const float* rows, const float* axes, float fx, int W, int H, float* rect) {
  for (int k = 0; k < n; k++) {
    const float* a = axes + 9 * (size_t)k;
    hd_pixel_rect(rows + 16 * (size_t)k, hv_mk(a[0], a[1], a[2]), hv_mk(a[3], a[4], a[5]), hv_mk(a[6], a[7], a[8]), fx, W, H,
                  rect + 4 * (size_t)k);
  }
}
