"""Single-product operands for the bf16-split GEMMs (csrc/hg_gemm.hip), test infrastructure only.

The bf16-split kernels write every f32 operand as three bf16 planes x = x0 + x1 + x2 (exact) and
keep six of the nine plane products, a0 b0 + a0 b1 + a1 b0 + a0 b2 + a1 b1 + a2 b0.  A dense test
bounds the result by 1e-6 sum_k |a_k b_k|, which grows with K while the error of one lost
second-order term grows like sqrt(K): above K ~ 200 a term lost in one staging path, one k group or
one plane of an image goes unseen.  Here one operand has a SINGLE non-zero per row, at k = row % K,
and the other is dense: every output element is exactly one product a b (the other K - 1 addends
are exact zeros), the rows between them visit every k of the reduction in one launch, and nothing
averages.

The bound is derived, not measured (rounding to nearest into 8 significant bits):
  * |x1| <= 2^-9 |x|, |x2| <= 2^-18 |x| (up to the position of x in its binade), x0 + x1 + x2 = x;
  * the dropped a1 b2 + a2 b1 + a2 b2 are at most about 2^-26 |a b|;
  * each bf16 x bf16 product is exact in f32;
  * the six accumulations round at most 6 times by 2^-24 of partial sums <= 1.01 |a b|;
  * total <= 6.3 x 2^-24 |a b|, asserted as  |y - a b| <= 2^-21 |a b|  (BOUND, 4.77e-7).
A reference of exactly 0 (a k outside a split-K slice) must come out as exactly 0.  On the f32 MFMA
tiles the result is one f32 product rounded once: |y - a b| <= 2^-23 |a b| (ULP), one unit in the
last place, whichever way the hardware rounds; HALF_ULP is what round-to-nearest would give.

split_model() is the CPU emulation of the kernels' arithmetic with the list of kept terms (and a
per-k mask for each) as arguments: tests/test_gemm_cases.py shows with it that the six-term model
passes check() and that every variant with a lower-order term, a plane or one chunk's term missing
does not.  tests/test_gpu_gemm_terms.py holds the kernels to the same check().
"""
import collections

import torch

BOUND = 2.0 ** -21     # six-term bf16-split product, relative to |a b|
ULP = 2.0 ** -23       # one f32 product rounded once, either rounding mode
HALF_ULP = 2.0 ** -24  # the same under round-to-nearest (reported, not asserted)

# (plane of a, plane of b) in the kernels' accumulation order, smallest first
TERMS6 = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
SECOND_ORDER = ((2, 0), (1, 1), (0, 2))
SIDES = ("A", "B")
ALIGNS = (16, 4)  # bytes: the float4 (VEC) staging; rows whose stride is no multiple of 4 floats

# (M, N, K) of C [M, N] = A [M, K] B [N, K]^T: M and N >= K, so either side's rows reach every k.
# 705 / 219: the observation widths (4-byte-aligned rows, a k tail of 1 / 11); 512: no tail; 33: two
# full chunks and a one-element tail; M and N are no multiple of any block tile
FWD_CASES = [(737, 709, 705), (260, 224, 219), (520, 520, 512), (40, 36, 33)]
# input gradient C [M, N] = A [M, K] B [K, N]: reduction 256 (no tail) and 40 (a tail of 8)
DX_CASES = [(261, 259, 256), (65, 129, 40)]
# split-K forward: with S slices of kslice = ceil16(ceil(K / S)) the slice boundary falls inside a
# 32-deep chunk pair (kslice / 16 odd) and the last slice is short at K = 705 (S 2, 3), 219 (S 2,
# 3), 150 (S 2, 4) and 33 (S 2, 3: a last slice of one element); tests/test_gemm_cases.py checks it
SPLITK_CASES = [(737, 709, 705), (260, 224, 219), (160, 152, 150), (40, 36, 33)]
SPLITK_S = (2, 3, 4)
# weight gradient (R, M, N, S): C_s [M, N] = sum_{r in slice s} A[r][m] B[r][n].  The one-hot side
# has its non-zero at reduction row col % R and reaches every r only with >= R columns: side A in
# the first three, side B in the last (the other side still runs, on the r it has)
WG_CASES = [(250, 257, 66, 1), (250, 257, 66, 3), (250, 257, 66, 40), (100, 66, 130, 2)]

OneHot = collections.namedtuple("OneHot", "a b side kidx")


def kslice(K, S, unit=16):
    """Reduction rows per split-K slice (hg_gemm_splitk_kslice; the image weight gradient: unit 32)."""
    return ((K + S - 1) // S + unit - 1) // unit * unit


def _randn24(shape, gen):
    """randn rounded from float64 with the last significand bit set: the value needs all 24 bits."""
    x = torch.randn(shape, generator=gen, dtype=torch.float64).float()
    return (x.view(torch.int32) | 1).view(torch.float32)


def _hot_values(rows, gen):
    """The one-hot operand's non-zeros: randn24 values kept only where both lower planes are within
    4 x of their largest size (|x1| >= 2^-11 |x|, |x2| >= 2^-20 |x|).  A k that only a few rows reach
    (the one-element tail of K = 33) then shows a lost plane of THIS operand on every one of them:
    the missing a0 b2 alone is >= 2^-20 |a b|, the six-term rounding <= 6.3 x 2^-24 |a b|, so the
    error stays above the 2^-21 bound whatever the dense partner holds."""
    x = _randn24((8 * rows + 64,), gen)
    _, x1, x2 = split(x)
    keep = (x1.abs() >= 2.0 ** -11 * x.abs()) & (x2.abs() >= 2.0 ** -20 * x.abs())
    x = x[keep]
    assert x.numel() >= rows
    return x[:rows]


def one_hot(rows, K, seed, side, dense_rows=None):
    """The operands of C = a b^T as (row, k) matrices, a [M, K] and b [N, K], on the CPU: side
    ("A" or "B") has `rows` rows with one non-zero each, row r's at k = r % K; the other operand is
    dense with `dense_rows` rows (default `rows`).  kidx[r] is the k of the one-hot side's row r."""
    assert side in SIDES
    gen = torch.Generator().manual_seed(seed)
    dense = _randn24((dense_rows or rows, K), gen)
    vals = _hot_values(rows, gen)
    kidx = torch.arange(rows) % K
    hot = torch.zeros(rows, K)
    hot[torch.arange(rows), kidx] = vals
    a, b = (hot, dense) if side == "A" else (dense, hot)
    return OneHot(a, b, side, kidx)


def embed(x, align, device=None):
    """x [R, C] as a row and column slice of a taller, wider NaN table: what lies before, after
    and between the operand's rows is poison, so a read outside it shows in the output.
    align 16: the slice starts 16-byte aligned and the row stride is a multiple of 4 floats (the
    float4 staging); align 4: column offset 3 and a row stride that is no multiple of 4 (every row
    starts at another 16-byte phase).  Returns (table, view)."""
    R, C = x.shape
    if align == 16:
        top, left = 2, 4
        ld = (C + left + 5 + 3) // 4 * 4
    else:
        assert align == 4
        top, left = 1, 3
        ld = C + left + 6
        ld += ld % 4 == 0
    table = torch.full((top + R + 2, ld), float("nan"), dtype=torch.float32, device=device or x.device)
    view = table[top:top + R, left:left + C]
    view.copy_(x)
    if align == 16:
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0
    else:
        assert view.data_ptr() % 4 == 0 and view.stride(0) % 4 != 0
    return table, view


def split(x, planes=3):
    """The three bf16 planes of x as f32 tensors (round to nearest even); planes = 2: the third
    plane never written."""
    x0 = x.to(torch.bfloat16).float()
    r1 = x - x0
    x1 = r1.to(torch.bfloat16).float()
    r2 = r1 - x1
    x2 = r2.to(torch.bfloat16).float() if planes >= 3 else torch.zeros_like(x)
    return x0, x1, x2


def split_model(a, b, terms=TERMS6, planes=3, kmask=None):
    """The kernels' arithmetic on a [M, K], b [N, K]: the plane products of `terms` ((i, j): a_i
    b_j) summed over k in float64 (exact under a one-hot operand), rounded to f32 and accumulated
    in f32 in the kernels' order, smallest first.  kmask {term: bool [K]} keeps a term only at the
    k where its mask is set (a term lost in one chunk or one k group)."""
    pa, pb = split(a, planes), split(b, planes)
    kmask = kmask or {}
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for t in TERMS6:
        if t not in terms:
            continue
        ai = pa[t[0]]
        if t in kmask:
            ai = ai * kmask[t].to(ai.dtype)[None, :]
        acc = acc + (ai.double() @ pb[t[1]].double().t()).float()
    return acc


def reference(a, b, S=1, ks=None):
    """The float64 product a b^T, exact under a one-hot operand; S > 1: [S, M, N], slice s the
    product over k in [s ks, (s + 1) ks) (exact zeros where the element's k lies elsewhere)."""
    a64, b64 = a.double(), b.double()
    if S == 1:
        return a64 @ b64.t()
    K = a.shape[1]
    sl = torch.arange(K, device=a.device) // ks
    return torch.stack([(a64 * (sl == s).to(a64.dtype)[None, :]) @ b64.t() for s in range(S)])


def measure(got, ref, side, K, bound=BOUND):
    """got against ref (the trailing two dimensions are [M, N]): the worst |got - ref| / (bound
    |ref|) over the elements with a non-zero reference, with its row, column and k, and the counts
    of elements over the bound and of zero-reference elements that are not exactly 0.  A NaN counts
    as over the bound."""
    got64 = got.double()
    nz = ref != 0
    lim = bound * ref.abs()
    err = (got64 - ref).abs()
    ratio = torch.where(nz, err / torch.where(nz, lim, torch.ones_like(lim)), torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    over = nz & ~(err <= lim)
    nonzero = ~nz & ~(got64 == 0)
    flat = int(ratio.reshape(-1).argmax())
    N = ref.shape[-1]
    M = ref.shape[-2]
    row, col = (flat // N) % M, flat % N
    return {"ratio": float(ratio.reshape(-1)[flat]), "row": row, "col": col, "slice": flat // (M * N),
            "k": (row if side == "A" else col) % K, "over": int(over.sum()), "nonzero": int(nonzero.sum()),
            "count": int(nz.sum()), "zeros": int((~nz).sum())}


def check(got, a, b, side="A", bound=BOUND, ref=None):
    """The violations of the per-product bound and of the exact zeros, as a list of strings (empty:
    got passes).  a [M, K], b [N, K] with side's operand one-hot; ref: a precomputed reference()."""
    if ref is None:
        ref = reference(a, b)
    m = measure(got, ref, side, a.shape[1], bound)
    out = []
    if m["over"]:
        out.append(f"{m['over']} of {m['count']} products over {bound:.3g} |ab|: worst {m['ratio']:.3g} x the bound "
                   f"at row {m['row']} column {m['col']} slice {m['slice']} (k = {m['k']})")
    if m["nonzero"]:
        out.append(f"{m['nonzero']} of {m['zeros']} elements with a zero reference are not exactly 0")
    return out
