"""Every term of the bf16-split GEMMs (csrc/hg_gemm.hip) on single-product operands.

tests/test_gpu_gemm.py bounds every form by 1e-6 sum_k |a_k b_k|; above K ~ 200 that bound is
larger than a lost second-order term (a0 b2, a1 b1, a2 b0), so a term missing in one staging path,
one k group, one plane of an image or one split-K slice passes it.  Here one operand has a single
non-zero per row, at k = row % K (oracle/gemm_cases.py): each output element is exactly one
product, the rows visit every k in one launch, and the result is held to the derived bound
|y - a b| <= 2^-21 |a b| (elements whose reference is 0, the other split-K slices, exactly 0).
tests/test_gemm_cases.py shows on the CPU model that the six-term arithmetic keeps that bound with
room and that no variant with a term, a plane or one chunk's term missing does.

Every case runs with side A one-hot and with side B one-hot, act 0 and no bias (a zero bias where
the entry needs one), from row and column slices of NaN tables at both alignments (16-byte: the
float4 staging; 4-byte with a row stride that is no multiple of 4), through every entry and every
tile id it accepts.  The f32 MFMA tiles 1..18 compute one f32 product rounded once and are held to
one ulp.  The last three tests scale the dense ragged operands of tests/test_gpu_gemm.py by 2^s and
2^-s: bf16 rounding commutes with a power of two, the plane products are the same real numbers,
and the output bits must not change (bias and ELU on).

Every passing case prints its worst ratio to the bound (pytest -s); a failure names entry, tile,
form, side, alignment, and row, column and k of the worst element.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as GC
from test_gpu_gemm import CASES, DX_CASES, WG_CASES, _need_gpu, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
X6 = range(19, 30)       # hg_gemm_f32: the bf16-split tiles (29 = 23 here)
X6_IMG = range(19, 33)   # the image entries: + the occupancy tiles 30 / 31 / 32
F32 = range(1, 19)       # the f32 MFMA tiles
SPLITK = range(20, 29)
SPLITK_IMG = (19, 20, 21, 22, 23, 25, 27, 28, 30, 31, 32)
WG_TR = range(40, 55)
WORST = {}


def _lib():
    _need_gpu()
    from humanoid import _native as N
    return N.lib()


class _Ops:
    """One case's operands on the device: compact a [M, K] and b [N, K], the float64 reference
    (never written again), and on demand their NaN-surrounded slices, plain or transposed."""

    def __init__(self, M, N, K, side):
        rows, dense = (M, N) if side == "A" else (N, M)
        c = GC.one_hot(rows, K, 1000 * M + N + K, side, dense)
        self.M, self.N, self.K, self.side = M, N, K, side
        self.a, self.b = c.a.to(DEV), c.b.to(DEV)
        self.ref = GC.reference(self.a, self.b)
        self._emb = {}

    def emb(self, name, align, trans=False):
        key = (name, align, trans)
        if key not in self._emb:
            x = getattr(self, name)
            self._emb[key] = GC.embed(x.t() if trans else x, align, DEV)
        return self._emb[key][1]


@functools.lru_cache(maxsize=None)
def _ops(M, N, K, side):
    return _Ops(M, N, K, side)


def _report(got, ops, entry, tile, form, align, bound=GC.BOUND, ref=None, extra=""):
    ref = ops.ref if ref is None else ref
    m = GC.measure(got, ref, ops.side, ops.K, bound)
    tag = (f"{entry} tile {tile} form {form} side {ops.side} align {align} shape "
           f"{(ops.M, ops.N, ops.K)}{extra}")
    assert m["count"] == ops.M * ops.N, tag  # every element is one product (in exactly one slice)
    if m["over"] or m["nonzero"]:
        pytest.fail(f"{tag}: " + "; ".join(GC.check(got, ops.a, ops.b, ops.side, bound, ref)))
    print(f"gemm_terms {tag}: worst ratio {m['ratio']:.3f} (row {m['row']} column {m['col']} k {m['k']})")
    WORST[entry] = max(WORST.get(entry, 0.0), m["ratio"])
    return m["ratio"]


def _summary(*entries):
    for e in entries:
        if e in WORST:
            print(f"gemm_terms worst so far, {e}: {WORST[e]:.3f} of its bound")


def _out(M, N, fill=7.0):
    return torch.full((M, N + 3), fill, device=DEV)  # strided output: the pad columns stay untouched


def _pad_ok(out, N, fill=7.0):
    return bool((out[..., N:] == fill).all())


def _image(L, P, trans, rows, k):
    img = torch.full((int(L.hg_gemm_x6_image_bytes(rows, k)) // 4,), float("nan"), device=DEV)
    vp = ctypes.c_void_p
    rc = L.hg_gemm_x6_image_jobs((vp * 1)(P.data_ptr()), (ctypes.c_int64 * 1)(P.stride(0)), (ctypes.c_int * 1)(trans),
                                 (ctypes.c_int64 * 1)(rows), (ctypes.c_int64 * 1)(k), (vp * 1)(img.data_ptr()), 1,
                                 _stream())
    assert rc == 0
    return img


def _nb(img):
    return img.numel() * img.element_size()


def _compact(x):
    """x [R, C] in the corner of a contiguous zero table: what an image reads past R and C is 0."""
    t = torch.zeros(x.shape[0] + 8, x.shape[1] + 8, device=DEV)
    t[:x.shape[0], :x.shape[1]] = x
    return t


def _images(L, ops, name, rows):
    """The operand image of a / b [rows, K], built from the NaN-surrounded slice in both trans
    settings and both alignments: each has the bytes of the image of a compact zero-padded copy."""
    x = getattr(ops, name)
    want = _image(L, _compact(x), 0, rows, ops.K)
    wint = want.view(torch.int32)
    assert torch.equal(wint, _image(L, _compact(x.t()), 1, rows, ops.K).view(torch.int32))
    for align in GC.ALIGNS:
        for trans in (0, 1):
            got = _image(L, ops.emb(name, align, bool(trans)), trans, rows, ops.K)
            assert torch.equal(got.view(torch.int32), wint), f"image of {name} trans {trans} align {align} side {ops.side}"
    return want


def _gemm(L, mode, A, B, M, N, K, tile, act=0, bias=None, Y=None, cp=None):
    out = _out(M, N)
    rc = L.hg_gemm_f32(mode, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0),
                       None if bias is None else bias.data_ptr(), None if Y is None else Y.data_ptr(),
                       0 if Y is None else Y.stride(0), out.data_ptr(), out.stride(0),
                       None if cp is None else cp.data_ptr(), M, N, K, act, tile, _stream())
    assert rc == 0, (mode, tile)
    return out


def _gemm_img(L, mode, A, aimg, bimg, M, N, K, tile, act=0, bias=None, Y=None, cp=None):
    out = _out(M, N)
    rc = L.hg_gemm_f32_img(mode, None if A is None else A.data_ptr(), 0 if A is None else A.stride(0),
                           None if aimg is None else aimg.data_ptr(), bimg.data_ptr(),
                           None if bias is None else bias.data_ptr(), None if Y is None else Y.data_ptr(),
                           0 if Y is None else Y.stride(0), out.data_ptr(), out.stride(0),
                           None if cp is None else cp.data_ptr(), M, N, K, act, tile,
                           0 if aimg is None else _nb(aimg), _nb(bimg), _stream())
    assert rc == 0, (mode, tile)
    return out


def _splitk(L, A, B, bimg, bias, M, N, K, tile, S, act=0):
    ws = torch.full((S * M * N,), float("nan"), device=DEV)  # every slice element is written before it is read
    out = _out(M, N)
    if bimg is None:
        rc = L.hg_gemm_f32_splitk(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), bias.data_ptr(), out.data_ptr(),
                                  out.stride(0), ws.data_ptr(), ws.numel(), M, N, K, act, tile, S, _stream())
    else:
        rc = L.hg_gemm_f32_splitk_img(A.data_ptr(), A.stride(0), bimg.data_ptr(), _nb(bimg), bias.data_ptr(),
                                      out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), M, N, K, act, tile, S,
                                      _stream())
    assert rc == 0, (tile, S)
    return out


def _wgrad(L, A, B, M, N, R, S, kmajor, tile):
    part = torch.full((S, M, N + 3), 5.0, device=DEV)
    rc = L.hg_gemm_f32_wgrad(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), part.data_ptr(), N + 3,
                             M * (N + 3), M, N, R, S, kmajor, tile, _stream())
    assert rc == 0, (kmajor, tile)
    return part


def _wgrad_img(L, ai, bi, M, N, R, S, tile):
    part = torch.full((S, M, N + 3), 5.0, device=DEV)
    rc = L.hg_gemm_wgrad_img(ai.data_ptr(), bi.data_ptr(), part.data_ptr(), N + 3, M * (N + 3), M, N, R, S, tile,
                             _nb(ai), _nb(bi), _stream())
    assert rc == 0, tile
    return part


# ---------------------------------------------------------------------------------------------
# one product per output element

@pytest.mark.parametrize("M,N,K", GC.FWD_CASES)
def test_forward_terms(M, N, K):
    """hg_gemm_f32 mode 0, tiles 19..29: both operands k-contiguous (X6Stage, VEC and unaligned)."""
    L = _lib()
    for side in GC.SIDES:
        ops = _ops(M, N, K, side)
        for align in GC.ALIGNS:
            A, B = ops.emb("a", align), ops.emb("b", align)
            for tile in X6:
                out = _gemm(L, 0, A, B, M, N, K, tile)
                _report(out[:, :N], ops, "hg_gemm_f32 mode 0", tile, "staged", align)
                assert _pad_ok(out, N)
    _summary("hg_gemm_f32 mode 0")


@pytest.mark.parametrize("M,N,K", GC.DX_CASES)
def test_input_grad_terms(M, N, K):
    """hg_gemm_f32 mode 1 (B [K, N] n-contiguous, through the LDS transpose scratch) and mode 3 (B
    [N, K] k-contiguous), tiles 19..29, act 0: the plain product."""
    L = _lib()
    for side in GC.SIDES:
        ops = _ops(M, N, K, side)
        for align in GC.ALIGNS:
            A = ops.emb("a", align)
            for mode, B in ((1, ops.emb("b", align, True)), (3, ops.emb("b", align))):
                for tile in X6:
                    out = _gemm(L, mode, A, B, M, N, K, tile)
                    _report(out[:, :N], ops, f"hg_gemm_f32 mode {mode}", tile, "staged", align)
                    assert _pad_ok(out, N)
    _summary("hg_gemm_f32 mode 1", "hg_gemm_f32 mode 3")


@pytest.mark.parametrize("M,N,K", GC.FWD_CASES + GC.DX_CASES)
def test_image_form_terms(M, N, K):
    """hg_gemm_f32_img modes 0 and 1, tiles 19..32 (29: A two chunks ahead; 30..32: the occupancy
    kernels), B from its image with A staged at both alignments, and both from their images; the
    images built from the NaN-surrounded operands have the bytes of a compact copy's."""
    L = _lib()
    for side in GC.SIDES:
        ops = _ops(M, N, K, side)
        aimg, bimg = _images(L, ops, "a", M), _images(L, ops, "b", N)
        for mode in (0, 1):  # the same images serve both: mode 1's W [K, N] is the trans 1 source of b's
            for tile in X6_IMG:
                for align in GC.ALIGNS:
                    out = _gemm_img(L, mode, ops.emb("a", align), None, bimg, M, N, K, tile)
                    _report(out[:, :N], ops, f"hg_gemm_f32_img mode {mode}", tile, "b_image", align)
                    assert _pad_ok(out, N)
                out = _gemm_img(L, mode, None, aimg, bimg, M, N, K, tile)
                _report(out[:, :N], ops, f"hg_gemm_f32_img mode {mode}", tile, "ab_image", "image")
                assert _pad_ok(out, N)
    _summary("hg_gemm_f32_img mode 0", "hg_gemm_f32_img mode 1")


@pytest.mark.parametrize("M,N,K", GC.SPLITK_CASES)
def test_splitk_terms(M, N, K):
    """hg_gemm_f32_splitk (tiles 20..28) and hg_gemm_f32_splitk_img (the tiles it accepts), 2 to 4
    slices wherever hg_gemm_splitk_kslice leaves none empty: slice boundaries inside a 32-deep
    chunk pair, a short last slice, the workspace NaN before every call."""
    L = _lib()
    bias = torch.zeros(N, device=DEV)
    ran = 0
    for side in GC.SIDES:
        ops = _ops(M, N, K, side)
        bimg = _images(L, ops, "b", N)
        for S in GC.SPLITK_S:
            ks = int(L.hg_gemm_splitk_kslice(K, S))
            assert ks == GC.kslice(K, S)
            if (S - 1) * ks >= K:
                continue
            for align in GC.ALIGNS:
                A, B = ops.emb("a", align), ops.emb("b", align)
                for tile in SPLITK:
                    out = _splitk(L, A, B, None, bias, M, N, K, tile, S)
                    _report(out[:, :N], ops, "hg_gemm_f32_splitk", tile, "staged", align, extra=f" S {S}")
                    assert _pad_ok(out, N)
                for tile in SPLITK_IMG:
                    out = _splitk(L, A, None, bimg, bias, M, N, K, tile, S)
                    _report(out[:, :N], ops, "hg_gemm_f32_splitk_img", tile, "b_image", align, extra=f" S {S}")
                    assert _pad_ok(out, N)
                ran += 1
    assert ran >= 8  # S = 2 and at least one more slice count, both sides and alignments
    _summary("hg_gemm_f32_splitk", "hg_gemm_f32_splitk_img")


@pytest.mark.parametrize("R,M,N,S", GC.WG_CASES)
def test_wgrad_terms(R, M, N, S):
    """hg_gemm_f32_wgrad: reduction-major operands (kmajor 0: the LDS transpose scratch; tiles
    40..54: k_wgrad_tr's transposed LDS reads) and k-contiguous ones (kmajor 1), and
    hg_gemm_wgrad_img from the two images.  Every slice is checked on its own: the product where
    the element's reduction row lies in the slice, exactly 0 elsewhere; and so is their sum."""
    L = _lib()
    for side in GC.SIDES:
        ops = _ops(M, N, R, side)
        ref = {u: GC.reference(ops.a, ops.b, S, GC.kslice(R, S, u)) if S > 1 else ops.ref[None] for u in (16, 32)}

        def both(part, entry, tile, form, align, unit=16):
            _report(part[:, :, :N], ops, entry, tile, form, align, ref=ref[unit], extra=f" S {S}")
            _report(part[:, :, :N].double().sum(0), ops, entry + " (slices summed)", tile, form, align, extra=f" S {S}")
            assert _pad_ok(part, N, 5.0)

        for align in GC.ALIGNS:
            At, Bt = ops.emb("a", align, True), ops.emb("b", align, True)  # [R, M], [R, N]
            A, B = ops.emb("a", align), ops.emb("b", align)
            for tile in range(19, 29):
                both(_wgrad(L, At, Bt, M, N, R, S, 0, tile), "hg_gemm_f32_wgrad kmajor 0", tile, "staged", align)
                both(_wgrad(L, A, B, M, N, R, S, 1, tile), "hg_gemm_f32_wgrad kmajor 1", tile, "staged", align)
            for tile in WG_TR:
                both(_wgrad(L, At, Bt, M, N, R, S, 0, tile), "hg_gemm_f32_wgrad tr", tile, "staged", align)
        ai, bi = _images(L, ops, "a", M), _images(L, ops, "b", N)
        for tile in range(19, 29):
            both(_wgrad_img(L, ai, bi, M, N, R, S, tile), "hg_gemm_wgrad_img", tile, "ab_image", "image", 32)
    _summary("hg_gemm_f32_wgrad kmajor 0", "hg_gemm_f32_wgrad kmajor 1", "hg_gemm_f32_wgrad tr", "hg_gemm_wgrad_img")


@pytest.mark.parametrize("M,N,K", GC.FWD_CASES + GC.DX_CASES)
def test_f32_mfma_tiles_round_one_product_once(M, N, K):
    """Tiles 1..18 (v_mfma_f32_32x32x2_f32) on the one-hot cases, modes 0 and 1: a single f32 product
    rounded once, within one ulp under either rounding mode; whether half an ulp held is printed."""
    L = _lib()
    half = True
    for side in GC.SIDES:
        ops = _ops(M, N, K, side)
        for align in GC.ALIGNS:
            A = ops.emb("a", align)
            for mode, B in ((0, ops.emb("b", align)), (1, ops.emb("b", align, True))):
                for tile in F32:
                    out = _gemm(L, mode, A, B, M, N, K, tile)
                    r = _report(out[:, :N], ops, f"hg_gemm_f32 mode {mode} f32 MFMA", tile, "staged", align, bound=GC.ULP)
                    half = half and r <= 0.5
                    assert _pad_ok(out, N)
    print(f"gemm_terms f32 MFMA tiles {(M, N, K)}: half an ulp (2^-24) {'held' if half else 'did NOT hold'} everywhere")
    _summary("hg_gemm_f32 mode 0 f32 MFMA", "hg_gemm_f32 mode 1 f32 MFMA")


# ---------------------------------------------------------------------------------------------
# power-of-two scaling: A 2^s, B 2^-s leaves every output bit as it was

SCALES = (40, -40)
SMALL = 1000  # rows: the small dense cases of tests/test_gpu_gemm.py


def _same(base, scaled, what):
    assert base.keys() == scaled.keys()
    for key in base:
        for t0, t1 in zip(base[key], scaled[key]):
            if not torch.equal(t0, t1):
                d = t0 != t1
                i = int(d.reshape(-1).nonzero()[0])
                pytest.fail(f"{what}: {key} changes {int(d.sum())} of {d.numel()} elements, first at flat index {i}: "
                            f"{t0.reshape(-1)[i].item()!r} -> {t1.reshape(-1)[i].item()!r}")
    print(f"gemm_terms scaling {what}: {len(base)} outputs bit for bit")


@pytest.mark.parametrize("rows,k,n,pad", [c for c in CASES if c[0] <= SMALL])
def test_scaling_forward_bits(rows, k, n, pad):
    L = _lib()
    torch.manual_seed(rows + k + n)
    xs = torch.randn(rows, k + pad, device=DEV)
    W = torch.randn(n, k, device=DEV) / k ** 0.5
    b = torch.randn(n, device=DEV) * 0.1

    def run(xs, W):
        x = xs[:, :k]
        res = {}
        for tile in list(F32) + list(X6):
            res["hg_gemm_f32 mode 0", tile] = (_gemm(L, 0, x, W, rows, n, k, tile, 1, b),)
        aimg, bimg = _image(L, x, 0, rows, k), _image(L, W, 0, n, k)
        for tile in X6_IMG:
            res["b_image", tile] = (_gemm_img(L, 0, x, None, bimg, rows, n, k, tile, 1, b),)
            res["ab_image", tile] = (_gemm_img(L, 0, None, aimg, bimg, rows, n, k, tile, 1, b),)
        for S in GC.SPLITK_S:
            if (S - 1) * int(L.hg_gemm_splitk_kslice(k, S)) >= k:
                continue
            for tile in SPLITK:
                res["splitk", tile, S] = (_splitk(L, x, W, None, b, rows, n, k, tile, S, 1),)
            for tile in SPLITK_IMG:
                res["splitk_img", tile, S] = (_splitk(L, x, None, bimg, b, rows, n, k, tile, S, 1),)
        return res

    base = run(xs, W)
    for s in SCALES:
        _same(base, run(xs * 2.0 ** s, W * 2.0 ** -s), f"forward {(rows, k, n)} s {s}")


@pytest.mark.parametrize("rows,kr,n", [c for c in DX_CASES if c[0] <= SMALL])
def test_scaling_input_grad_bits(rows, kr, n):
    L = _lib()
    torch.manual_seed(rows + kr + n)
    g = torch.randn(rows, kr, device=DEV)
    W = torch.randn(kr, n, device=DEV) / kr ** 0.5
    y = F.elu(torch.randn(rows, n, device=DEV))

    def run(g, W):
        Wt = W.t().contiguous()
        res = {}

        def cp(tile):
            return torch.full((int(L.hg_gemm_colpart_rows(rows, tile)), n), float("nan"), device=DEV)

        for tile in list(F32) + list(X6):
            for mode, B in ((1, W), (3, Wt)):
                if mode == 3 and tile < 19:
                    continue
                c = cp(tile)
                res[f"hg_gemm_f32 mode {mode}", tile] = (_gemm(L, mode, g, B, rows, n, kr, tile, 1, None, y, c), c)
        aimg, bimg = _image(L, g, 0, rows, kr), _image(L, W, 1, n, kr)
        for tile in X6_IMG:
            c = cp(tile)
            res["b_image", tile] = (_gemm_img(L, 1, g, None, bimg, rows, n, kr, tile, 1, None, y, c), c)
            c = cp(tile)
            res["ab_image", tile] = (_gemm_img(L, 1, None, aimg, bimg, rows, n, kr, tile, 1, None, y, c), c)
        return res

    base = run(g, W)
    for s in SCALES:
        _same(base, run(g * 2.0 ** s, W * 2.0 ** -s), f"input grad {(rows, kr, n)} s {s}")


@pytest.mark.parametrize("rows,n,k,S", [c for c in WG_CASES if c[0] <= SMALL])
def test_scaling_wgrad_bits(rows, n, k, S):
    L = _lib()
    torch.manual_seed(rows + n + k + S)
    gh = torch.randn(rows, n, device=DEV)
    x = torch.randn(rows, k, device=DEV)

    def run(gh, x):
        ght, xt = gh.t().contiguous(), x.t().contiguous()
        res = {}
        for tile in range(19, 29):
            res["kmajor 0", tile] = (_wgrad(L, gh, x, n, k, rows, S, 0, tile),)
            res["kmajor 1", tile] = (_wgrad(L, ght, xt, n, k, rows, S, 1, tile),)
        for tile in WG_TR:
            res["tr", tile] = (_wgrad(L, gh, x, n, k, rows, S, 0, tile),)
        ai, bi = _image(L, gh, 1, n, rows), _image(L, x, 1, k, rows)
        for tile in range(19, 29):
            res["wgrad_img", tile] = (_wgrad_img(L, ai, bi, n, k, rows, S, tile),)
        return res

    base = run(gh, x)
    for s in SCALES:
        _same(base, run(gh * 2.0 ** s, x * 2.0 ** -s), f"weight grad {(rows, n, k, S)} s {s}")
