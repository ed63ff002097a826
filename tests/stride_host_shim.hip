// Host build of the stride detector's sample (csrc/hg_stride_sample.h: hg_stride_sample_env and
// hg_stride_ground are __host__ __device__).  TEST INFRASTRUCTURE ONLY: tests/test_stride_cases.py
// compiles this file into a shared object, loads it with ctypes and runs the sample on the CPU
// against tests/stride_ref.py.  Nothing here launches a kernel.  HG_STRIDE_SRC names the header to
// include, so that the same shim builds the tree's sample and the one-line wrong samples the test
// writes into its tmp dir.
#include <hip/hip_runtime.h>

#ifndef HG_STRIDE_SRC
#define HG_STRIDE_SRC "../humanoid-gym-with-comments_amd/csrc/hg_stride_sample.h"
#endif
#include HG_STRIDE_SRC

// One sample for envs 0 .. n-1 of SoA arrays with row stride np (the arena's layout: root [13][np],
// contact [39][np], rigid [169][np]); state [16][np] and run [20][np] are updated in place.  hf: the
// heightfield [rows][cols] (NULL with terrain_type 0).  Returns how many envs took the sample.
extern "C" int stride_sample_host(int n, int np, const float* root, const float* contact, const float* rigid,
                                  const int32_t* feet, const int16_t* hf, int rows, int cols, float hs, float vs,
                                  float border, int terrain_type, double dt, double* state, double* run) {
  const HgStrideIn in = {root, contact, rigid};
  int taken = 0;
  for (int e = 0; e < n; e++)
    taken += hg_stride_sample_env(in, np, e, feet, hf, rows, cols, hs, vs, border, terrain_type, dt, state, run);
  return taken;
}

extern "C" double stride_ground_host(const int16_t* hf, int rows, int cols, float hs, float vs, float border,
                                     int terrain_type, double x, double y) {
  return hg_stride_ground(hf, rows, cols, hs, vs, border, terrain_type, x, y);
}
