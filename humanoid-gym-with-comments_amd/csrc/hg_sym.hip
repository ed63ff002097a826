// hg_sym.hip — the mirror-symmetry loss of the PPO update (gfx950).
//
// Replaces, on the device path, the reference's (humanoid/algo/ppo/ppo.py:197-202)
//   mirror_obs   = obs_batch @ obs_perm_mat          -> hg_mirror_rows (a signed column gather)
//   m_mirror_act = actor(mirror_obs) @ act_perm_mat
//   sym_loss     = (mu_batch - m_mirror_act).pow(2).mean()   -> hg_sym_loss (+ its gradients)
// The permutation matrices have one +-1 per column, so both products are signed column gathers:
// out[r][c] = sign[c] * in[r][perm[c]].
//
// hg_mirror_rows is HBM-bound: 2 x rows x width x 4 B (139 MB at 24576 x 705) and no arithmetic.
// A block owns MIRROR_ROWS consecutive rows; thread t owns the columns t, t + 256, ..: the table
// entry is read once per column and reused for the block's rows, the block's loads of one column
// chunk are all issued before its stores, and every wave stores 64 consecutive floats of a row
// (rows of 705 floats start on 4-byte boundaries only, so the stores are dword stores).  The
// reads are gathers inside one row: a row's cache lines are all consumed by the block that reads it.
//
// hg_sym_loss: one thread per row (as hg_ppo_loss), squares accumulated in float64, per-wave
// partials in scratch, one final block sums them in a fixed order — bitwise reproducible.
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hgsim.h"

namespace {
constexpr int MIRROR_TPB = 256;
constexpr int MIRROR_ROWS = 8;

__global__ void __launch_bounds__(MIRROR_TPB) k_mirror_rows(const float* __restrict__ src, int64_t src_ld,
                                                           float* __restrict__ dst, int64_t dst_ld, int64_t rows,
                                                           int width, const int32_t* __restrict__ perm,
                                                           const float* __restrict__ sign) {
  const int64_t r0 = (int64_t)blockIdx.x * MIRROR_ROWS;
  const int nr = rows - r0 < MIRROR_ROWS ? (int)(rows - r0) : MIRROR_ROWS;
  for (int c = threadIdx.x; c < width; c += MIRROR_TPB) {
    const int p = perm[c];
    const bool ok = (unsigned)p < (unsigned)width;  // an entry outside the row reads nothing: a zero column
    const float s = ok ? sign[c] : 0.f;
    const float* in = src + r0 * src_ld + (ok ? p : 0);
    float* out = dst + r0 * dst_ld + c;
    float v[MIRROR_ROWS];
#pragma unroll
    for (int k = 0; k < MIRROR_ROWS; k++) v[k] = k < nr ? in[k * src_ld] : 0.f;
#pragma unroll
    for (int k = 0; k < MIRROR_ROWS; k++)
      if (k < nr) out[k * dst_ld] = s * v[k];
  }
}

constexpr int SYM_TPB = 64;  // one wave per block: 384 blocks at the 24576-row minibatch

__global__ void __launch_bounds__(SYM_TPB) k_sym_rows(const float* __restrict__ mu, int64_t mu_ld,
                                                     const float* __restrict__ mir, int64_t mir_ld,
                                                     const int32_t* __restrict__ perm, const float* __restrict__ sign,
                                                     int64_t rows, int A, float c2, float* __restrict__ g_mu,
                                                     float* __restrict__ g_mir, double* __restrict__ partial) {
  const int64_t r = (int64_t)blockIdx.x * SYM_TPB + threadIdx.x;
  double acc = 0.0;
  if (r < rows) {
    const float* a = mu + r * mu_ld;
    const float* b = mir + r * mir_ld;
    for (int i = 0; i < A; i++) {
      const int p = perm[i];
      if ((unsigned)p >= (unsigned)A) continue;  // not a permutation: the caller's contract (hgsim.h)
      const float s = sign[i];
      const float d = a[i] - s * b[p];
      acc += (double)d * (double)d;
      const float g = c2 * d;
      g_mu[r * A + i] = g;
      g_mir[r * A + p] = -s * g;
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(64) k_sym_final(const double* __restrict__ partial, int nb, double count,
                                                 double coef, float* __restrict__ loss_out,
                                                 float* __restrict__ sym_out) {
  // lane l sums blocks l, l + 64, .. in order, then one fixed-order wave reduction
  double x = 0.0;
#pragma unroll 8
  for (int b = threadIdx.x; b < nb; b += 64) x += partial[b];
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  if (threadIdx.x == 0) {
    const double sym = x / count;
    sym_out[0] = (float)sym;
    loss_out[0] = (float)(coef * sym);
  }
}

__global__ void __launch_bounds__(256) k_sym_bwd(const float* __restrict__ g, int64_t n, float* __restrict__ g_mu,
                                                float* __restrict__ g_mir) {
  const float s = *g;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    g_mu[i] *= s;
    g_mir[i] *= s;
  }
}
}  // namespace

extern "C" int hg_mirror_rows(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int64_t rows, int width,
                              const int32_t* perm, const float* sign, void* stream) {
  if (!src || !dst || !perm || !sign || rows <= 0 || width <= 0 || src_ld < width || dst_ld < width || src == dst)
    return HG_ERR_ARG;
  const int64_t nb = (rows + MIRROR_ROWS - 1) / MIRROR_ROWS;
  if (nb > INT32_MAX) return HG_ERR_ARG;
  hipLaunchKernelGGL(k_mirror_rows, dim3((unsigned)nb), dim3(MIRROR_TPB), 0, (hipStream_t)stream, src, src_ld, dst,
                     dst_ld, rows, width, perm, sign);
  return hipGetLastError() == hipSuccess ? HG_OK : HG_ERR_HIP;
}

extern "C" int64_t hg_sym_loss_scratch(int64_t rows, int num_actions) {
  (void)num_actions;
  return rows > 0 ? (rows + SYM_TPB - 1) / SYM_TPB : 0;
}

extern "C" int hg_sym_loss(const float* mu, int64_t mu_ld, const float* mu_mirror, int64_t mu_mirror_ld,
                           const int32_t* perm, const float* sign, int64_t rows, int num_actions, double coef,
                           float* loss_out, float* sym_out, float* grad_mu, float* grad_mirror, double* scratch,
                           void* stream) {
  const int A = num_actions;
  if (!mu || !mu_mirror || !perm || !sign || !loss_out || !sym_out || !grad_mu || !grad_mirror || !scratch ||
      rows <= 0 || A <= 0 || A > HG_MAX_DOF || mu_ld < A || mu_mirror_ld < A)
    return HG_ERR_ARG;
  const int64_t nb64 = (rows + SYM_TPB - 1) / SYM_TPB;
  if (nb64 > INT32_MAX) return HG_ERR_ARG;
  const int nb = (int)nb64;
  const double count = (double)rows * (double)A;
  const float c2 = (float)(coef * 2.0 / count);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sym_rows, dim3(nb), dim3(SYM_TPB), 0, s, mu, mu_ld, mu_mirror, mu_mirror_ld, perm, sign, rows,
                     A, c2, grad_mu, grad_mirror, scratch);
  hipLaunchKernelGGL(k_sym_final, dim3(1), dim3(64), 0, s, scratch, nb, count, coef, loss_out, sym_out);
  return hipGetLastError() == hipSuccess ? HG_OK : HG_ERR_HIP;
}

extern "C" int hg_sym_loss_backward(const float* grad_loss, int64_t rows, int num_actions, float* grad_mu,
                                    float* grad_mirror, void* stream) {
  if (!grad_loss || rows <= 0 || num_actions <= 0 || !grad_mu || !grad_mirror) return HG_ERR_ARG;
  const int64_t n = rows * num_actions;
  const int nb = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(k_sym_bwd, dim3(nb), dim3(256), 0, (hipStream_t)stream, grad_loss, n, grad_mu, grad_mirror);
  return hipGetLastError() == hipSuccess ? HG_OK : HG_ERR_HIP;
}
