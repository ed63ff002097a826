"""The follow-camera view's plumbing without a GPU: hg_view_cam's layout, view_cam's refusals (every
one hg_render_view lists), the viewer config, the PNG writer / reader, and play.py's new flags."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_size_matches_header(tmp_path):
    from humanoid import _native as N
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hgsim.h"\nint main(){printf("%zu %zu %zu %zu %zu",'
                 'sizeof(hg_view_cam),offsetof(hg_view_cam,mode),offsetof(hg_view_cam,eye),'
                 'offsetof(hg_view_cam,target),offsetof(hg_view_cam,far_clip));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    C = N.HgViewCam
    assert got == [ctypes.sizeof(C), C.mode.offset, C.eye.offset, C.target.offset, C.far_clip.offset]
    assert "hg_render_view" in N.EXPORTS and "hg_view_shapes" in N.EXPORTS


def test_viewer_config_and_view_cam_refusals():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    v = XBotLCfg.viewer
    assert tuple(v.record_size) == (640, 360) and v.horizontal_fov == 60 and v.far_clip == 50.0
    assert list(v.follow_offset) == [2.0, -2.0, 0.8] and list(v.follow_target) == [0, 0, -0.2]
    assert list(v.pos) == [10, 0, 6] and list(v.lookat) == [11.0, 5, 3.0]      # the mode-0 default, kept
    cam = N.view_cam(v.record_size, v.horizontal_fov, v.follow_offset, v.follow_target, v.far_clip)
    assert (cam.width, cam.height, cam.mode, cam.horizontal_fov_deg, cam.far_clip) == (640, 360, 1, 60.0, 50.0)
    assert [cam.eye[k] for k in range(3)] == [2.0, -2.0, np.float32(0.8)]
    assert N.view_cam(v.record_size, 60, v.pos, v.lookat, 50.0, mode=0).mode == 0
    good = dict(size=(64, 36), horizontal_fov=60.0, eye=(2.0, -2.0, 0.8), target=(0.0, 0.0, -0.2), far_clip=50.0)

    def bad(**kw):
        with pytest.raises(ValueError):
            N.view_cam(**dict(good, **kw))
    N.view_cam(**good)
    bad(size=(0, 36))
    bad(size=(64, -1))
    bad(size=(1921, 1080))                      # W * H > 1920 * 1080
    N.view_cam(**dict(good, size=(1920, 1080)))  # the largest accepted
    bad(n=0)
    bad(n=-3)
    bad(size=(1920, 1080), n=1036)              # n * W * H >= 2^31
    N.view_cam(**dict(good, size=(1920, 1080), n=1035))
    bad(horizontal_fov=0.0)
    bad(horizontal_fov=180.0)
    bad(horizontal_fov=float("nan"))
    bad(far_clip=0.0)
    bad(far_clip=-1.0)
    bad(far_clip=float("inf"))
    bad(far_clip=float("nan"))
    bad(target=good["eye"])                     # eye equal to target
    bad(eye=(1.0, 2.0, 3.0), target=(1.0, 2.0, 5.0))   # looking along +z: no up vector
    bad(eye=(1.0, 2.0, 3.0), target=(1.0, 2.0, -5.0))  # ... or along -z
    bad(eye=(float("nan"), 0.0, 0.0))
    bad(mode=2)
    bad(eye=(1.0, 2.0))


def test_native_refusals_need_no_launch():
    """hg_render_view / hg_view_shapes refuse a NULL sim before anything else (CPU: nothing is launched)."""
    from humanoid import _native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    L = N.load_library()
    cam = N.view_cam((64, 36), 60.0, (2.0, -2.0, 0.8), (0.0, 0.0, -0.2), 50.0)
    fake = ctypes.c_void_p(0x10000)
    assert L.hg_render_view(None, ctypes.byref(cam), None, 1, fake, None, None, None) == 1
    assert b"sim" in L.hg_last_error(None)
    assert L.hg_view_shapes(None, None, 1, fake, None, None) == 1
    assert b"sim" in L.hg_last_error(None)


def test_png_round_trip(tmp_path):
    from humanoid.utils.png import read_chunks, read_png, write_png
    img = np.random.RandomState(11).randint(0, 256, (7, 9, 3)).astype(np.uint8)   # 9 wide, 7 high
    path = str(tmp_path / "a.png")
    write_png(path, img)
    assert np.array_equal(read_png(path), img)
    chunks = read_chunks(path)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (9, 7, 8, 2, 0, 0, 0)
    rows = zlib.decompress(chunks[1][1])
    want = b"".join(b"\x00" + img[r].tobytes() for r in range(7))   # filter byte 0 + the row
    assert rows == want
    for wrong in (img.astype(np.float32), img[:, :, :2], img[0]):
        with pytest.raises(ValueError):
            write_png(path, wrong)


def test_read_png_undoes_the_row_filters(tmp_path):
    """A file written with the Sub, Up, Average and Paeth filters (by this test) decodes to the image."""
    from humanoid.utils.png import _chunk, SIGNATURE, read_png
    img = np.random.RandomState(12).randint(0, 256, (5, 4, 3)).astype(np.int32)
    h, w = img.shape[:2]
    flat = img.reshape(h, 3 * w)
    raw = bytearray()
    for r in range(h):
        ft = [1, 2, 3, 4, 0][r]
        prev = flat[r - 1] if r else np.zeros(3 * w, np.int32)
        line = []
        for i in range(3 * w):
            a = flat[r, i - 3] if i >= 3 else 0
            b = prev[i]
            c = prev[i - 3] if i >= 3 else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            paeth = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            pred = [0, a, b, (a + b) // 2, paeth][ft]
            line.append((flat[r, i] - pred) & 255)
        raw += bytes([ft]) + bytes(line)
    path = str(tmp_path / "f.png")
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(bytes(raw))) + _chunk(b"IEND", b""))
    assert np.array_equal(read_png(path), img.astype(np.uint8))


def test_play_flags_parse_and_default_to_off():
    import inspect
    from humanoid.scripts import play as P
    extra, rest = P.record_parser().parse_known_args(["--task", "humanoid_ppo", "--steps", "7"])
    assert (extra.steps, extra.record, extra.record_env, extra.record_every) == (7, None, 0, 1)
    assert rest == ["--task", "humanoid_ppo"]
    extra, rest = P.record_parser().parse_known_args(["--record", "out", "--record_env", "3", "--record_every", "4", "--headless"])
    assert (extra.steps, extra.record, extra.record_env, extra.record_every) == (100, "out", 3, 4)
    assert rest == ["--headless"]
    sig = inspect.signature(P.play)
    assert list(sig.parameters)[:2] == ["args", "steps"] and sig.parameters["steps"].default == 100
    assert sig.parameters["record"].default is None
    assert sig.parameters["record_env"].default == 0 and sig.parameters["record_every"].default == 1
    assert "no renderer" not in P.__doc__
