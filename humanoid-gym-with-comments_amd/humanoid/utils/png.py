"""Minimal PNG writer / reader for 8-bit RGB images, standard library only (zlib, struct): what
play.py --record writes its frames with, so recording needs no imaging package."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, rgb_uint8_hwc, level=6):
    """Write a uint8 [H, W, 3] array as an 8-bit RGB PNG (filter type 0 on every row)."""
    a = np.asarray(rgb_uint8_hwc)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: need a uint8 [H, W, 3] array, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), np.uint8)  # column 0: the filter byte (0 = None)
    rows[:, 1:] = a.reshape(h, 3 * w)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)  # 8 bits, colour type 2 (RGB), no interlace
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level))
                + _chunk(b"IEND", b""))


def read_chunks(path):
    """[(tag, data)] of a PNG file; checks the signature and every CRC."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != SIGNATURE:
        raise ValueError(f"{path}: not a PNG file")
    out, at = [], 8
    while at < len(raw):
        n, = struct.unpack(">I", raw[at:at + 4])
        tag, data = raw[at + 4:at + 8], raw[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", raw[at + 8 + n:at + 12 + n])
        if crc != (zlib.crc32(tag + data) & 0xFFFFFFFF):
            raise ValueError(f"{path}: bad CRC in chunk {tag!r}")
        out.append((tag, data))
        at += 12 + n
    return out


def read_png(path):
    """uint8 [H, W, 3] of an 8-bit non-interlaced RGB PNG (any of the five row filters)."""
    chunks = read_chunks(path)
    if not chunks or chunks[0][0] != b"IHDR":
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, bits, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if (bits, ctype, comp, flt, lace) != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit non-interlaced RGB is supported")
    raw = zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT"))
    stride = 3 * w
    if len(raw) != h * (stride + 1):
        raise ValueError(f"{path}: image data has {len(raw)} bytes, expected {h * (stride + 1)}")
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for r in range(h):
        ft, line = int(rows[r, 0]), rows[r, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):  # these look left: byte by byte
            cur = np.zeros(stride, np.int32)
            for i in range(stride):
                a = cur[i - 3] if i >= 3 else 0
                b = prev[i]
                c = prev[i - 3] if i >= 3 else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        else:
            raise ValueError(f"{path}: bad filter type {ft} in row {r}")
        out[r] = cur
        prev = cur
    return out.reshape(h, w, 3)
