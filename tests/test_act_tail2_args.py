"""hg_gemm_f32_splitk_partials and hg_rollout_act_tail2 validate their arguments before any device
work (CPU: every call here is refused, nothing is launched)."""
import ctypes
import os

import pytest

from humanoid import _native as N


def _lib():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    return N.load_library()


def test_splitk_partials_rejects_bad_arguments():
    L = _lib()
    fake = ctypes.c_void_p(0x10000)  # 16-byte aligned, never dereferenced on a refused call
    args = dict(A=fake, lda=705, B=fake, ldb=705, ws=fake, wsf=4 * 4096 * 512, M=4096, N=512, K=705, tile=25, slices=4)

    def call(**kw):
        a = dict(args, **kw)
        return L.hg_gemm_f32_splitk_partials(a["A"], a["lda"], a["B"], a["ldb"], a["ws"], a["wsf"], a["M"], a["N"],
                                             a["K"], a["tile"], a["slices"], None)
    assert call(slices=1) != 0                     # not split
    assert call(slices=17) != 0
    assert call(K=16, lda=16, ldb=16) != 0         # an empty slice
    assert call(wsf=4 * 4096 * 512 - 1) != 0       # workspace short of slices x M x N
    assert call(ws=ctypes.c_void_p(0x10004)) != 0  # workspace not 16-byte aligned
    assert call(tile=5) != 0 and call(tile=29) != 0  # hg_gemm_f32_splitk's tiles only
    assert call(A=None) != 0 and call(B=None) != 0 and call(ws=None) != 0
    assert call(lda=704) != 0 and call(ldb=704) != 0
    assert call(M=0) != 0


def test_act_tail2_rejects_bad_arguments():
    L = _lib()
    fake = ctypes.c_void_p(0x10000)
    odd = ctypes.c_void_p(0x10004)
    n = 64
    lead = dict(ws=fake, wsf=4 * n * 512, slices=4, b1=fake, W2=fake, b2=fake, n1=512, n2=256, W3=fake, b3=fake, W=fake,
                b=fake)

    def call(num_envs=n, num_actions=12, **kw):
        a = dict(lead, **kw)
        return L.hg_rollout_act_tail2(a["ws"], a["wsf"], a["slices"], a["b1"], a["W2"], a["b2"], a["n1"], a["n2"],
                                      a["W3"], a["b3"], a["W"], a["b"], fake, None, fake, None, num_envs, num_actions,
                                      705, 0, 705, 0, 0, fake, fake, fake, fake, None, fake, 0, None, 0, 0, 1, 0, None)
    assert call(slices=2) != 0                      # the finish it replaces sums four slices
    assert call(n1=256) != 0 and call(n2=128) != 0  # 512 -> 256 only
    assert call(wsf=4 * n * 512 - 1) != 0           # workspace short of 4 x rows x 512
    for k in ("ws", "b1", "W2", "W3", "W"):         # read as float4
        assert call(**{k: odd}) != 0, k
    for k in ("ws", "b1", "W2", "b2", "W3", "b3", "W", "b"):
        assert call(**{k: None}) != 0, k
    assert call(num_actions=11) != 0                # the 12 x 128 head only
    assert call(num_envs=0) != 0
