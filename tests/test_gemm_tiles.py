"""The tile ids each GEMM entry of csrc/hg_gemm.hip takes, and the block rows hg_gemm_colpart_rows
sizes the column-partial buffer by (CPU: every entry call here is refused with HG_ERR_ARG before
any launch; an id let through by mistake would reach the launch and, with no device, return
HG_ERR_HIP or abort)."""
import ctypes
import os

import pytest

from humanoid import _native as N

HG_ERR_ARG = 1
IDS = range(0, 57)
F32 = set(range(1, 19))        # k_gemm
X6 = set(range(19, 33))        # k_gemm_x6 / k_gemm_x6_occ; 29..32 are image-only forms
STAGED = set(range(19, 29))    # the bf16-split tiles that are their own staged form
WGRAD_TR = set(range(40, 55))  # k_wgrad_tr

# block rows of tile ids 1..32
BM = [128, 128, 64, 64, 64, 64, 64, 128, 128, 128, 64, 128, 128, 64, 64, 128, 128, 64,
      64, 128, 128, 128, 64, 128, 256, 128, 128, 64, 64, 256, 128, 128]

M_, N_, K_ = 130, 96, 67
P = ctypes.c_void_p(0x10000)  # 16-byte aligned, never dereferenced on a refused call


def _lib():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    return N.load_library()


def test_colpart_rows_follow_each_tiles_block_rows():
    L = _lib()
    assert len(BM) == 32
    for tile in range(1, 33):
        for m in (1, 255, 256, 257):
            assert L.hg_gemm_colpart_rows(m, tile) == -(-m // BM[tile - 1]), (tile, m)
    for tile in (0, 33, 40):
        assert L.hg_gemm_colpart_rows(256, tile) == -1, tile


def _entries(L):
    """(name, accepted ids, call(tile)) for every entry that takes a tile id, arguments otherwise valid."""
    img_a, img_b = L.hg_gemm_x6_image_bytes(M_, K_), L.hg_gemm_x6_image_bytes(N_, K_)
    assert img_a > 0 and img_b > 0
    ws = 3 * M_ * N_
    n2, nsplit = 512, 256  # hg_gemm_f32_img_split: two outputs, the split a multiple of 256
    out = []
    for mode, ids in ((0, F32 | X6), (1, F32 | X6), (3, X6)):
        ldb = N_ if mode == 1 else K_
        out.append((f"hg_gemm_f32 mode {mode}", ids, lambda t, mode=mode, ldb=ldb: L.hg_gemm_f32(
            mode, P, K_, P, ldb, P, P, N_, P, N_, None, M_, N_, K_, 1, t, None)))
    for kmajor, ids in ((0, STAGED | WGRAD_TR), (1, STAGED)):
        lda, ldb = (K_, K_) if kmajor else (M_, N_)
        out.append((f"hg_gemm_f32_wgrad kmajor {kmajor}", ids, lambda t, kmajor=kmajor, lda=lda, ldb=ldb:
                    L.hg_gemm_f32_wgrad(P, lda, P, ldb, P, N_, M_ * N_, M_, N_, K_, 2, kmajor, t, None)))
    out.append(("hg_gemm_f32_splitk", STAGED - {19}, lambda t: L.hg_gemm_f32_splitk(
        P, K_, P, K_, P, P, N_, P, ws, M_, N_, K_, 1, t, 3, None)))
    out.append(("hg_gemm_f32_splitk_partials", STAGED - {19}, lambda t: L.hg_gemm_f32_splitk_partials(
        P, K_, P, K_, P, ws, M_, N_, K_, t, 3, None)))
    for mode in (0, 1):
        out.append((f"hg_gemm_f32_img mode {mode}, B image", X6, lambda t, mode=mode: L.hg_gemm_f32_img(
            mode, P, K_, None, P, P, P, N_, P, N_, None, M_, N_, K_, 1, t, 0, img_b, None)))
        out.append((f"hg_gemm_f32_img mode {mode}, A and B images", X6, lambda t, mode=mode: L.hg_gemm_f32_img(
            mode, None, 0, P, P, P, P, N_, P, N_, None, M_, N_, K_, 1, t, img_a, img_b, None)))
    out.append(("hg_gemm_f32_img_split", X6, lambda t: L.hg_gemm_f32_img_split(
        P, K_, P, P, P, P, nsplit, P, n2 - nsplit, nsplit, M_, n2, K_, 1, t, L.hg_gemm_x6_image_bytes(n2, K_), None)))
    out.append(("hg_gemm_wgrad_img", X6 - {30, 31, 32}, lambda t: L.hg_gemm_wgrad_img(
        P, P, P, N_, M_ * N_, M_, N_, K_, 2, t, img_a, img_b, None)))
    out.append(("hg_gemm_f32_splitk_img", X6 - {24, 26, 29}, lambda t: L.hg_gemm_f32_splitk_img(
        P, K_, P, img_b, P, P, N_, P, ws, M_, N_, K_, 1, t, 3, None)))
    return out


def test_every_entry_refuses_the_ids_outside_its_set():
    L = _lib()
    for name, accepted, call in _entries(L):
        for tile in IDS:
            if tile not in accepted:  # an accepted id is never called here: it would launch
                assert call(tile) == HG_ERR_ARG, (name, tile)
