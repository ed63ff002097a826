"""The single-product operands of oracle/gemm_cases.py, on the CPU model alone (no GPU).

tests/test_gpu_gemm_terms.py holds the bf16-split kernels to gemm_cases.check(); here the check
itself is held to what it promises, so the GPU test cannot pass on operands that would hide a lost
term:

  model      the six-term emulation of the kernels' arithmetic passes check() at every case shape
             and side, with room (worst ratio below 1/2 of the bound)
  mutants    each of the five one-term variants below a0 b0, and the split whose third plane is
             never written, breaks the bound on at least half of the elements; a second-order term
             dropped only in the last chunk, or only in k group 1 of 2, is still flagged
  coverage   the one-hot rows of every case reach every k of the reduction; the split-K cases put,
             for each slice count, a slice boundary inside a 32-deep chunk pair and end on a short
             slice; the embedded operands are surrounded by NaN at both alignments
"""
import pytest
import torch

import gemm_cases as GC

SHAPES = sorted(set(GC.FWD_CASES + GC.DX_CASES + GC.SPLITK_CASES + [(m, n, r) for r, m, n, _ in GC.WG_CASES]))


def _covers(M, N, K, side):
    return (M if side == "A" else N) >= K


def _case(M, N, K, side):
    rows, dense = (M, N) if side == "A" else (N, M)
    return GC.one_hot(rows, K, 1000 * M + N + K, side, dense)


@pytest.fixture(scope="module")
def cases():
    return {(s, side): _case(*s, side) for s in SHAPES for side in GC.SIDES}


@pytest.mark.parametrize("shape", SHAPES)
def test_six_term_model_passes(cases, shape):
    for side in GC.SIDES:
        c = cases[shape, side]
        got = GC.split_model(c.a, c.b)
        assert GC.check(got, c.a, c.b, side) == []
        m = GC.measure(got, GC.reference(c.a, c.b), side, shape[2])
        print(f"{shape} side {side}: six-term worst ratio {m['ratio']:.3f}")
        assert m["ratio"] < 0.5 and m["zeros"] == 0 and m["count"] == shape[0] * shape[1]


@pytest.mark.parametrize("shape", SHAPES)
def test_one_term_mutants_fail_on_half_the_elements(cases, shape):
    for side in GC.SIDES:
        c = cases[shape, side]
        ref = GC.reference(c.a, c.b)
        variants = [(f"without a{i}b{j}", dict(terms=[t for t in GC.TERMS6 if t != (i, j)]))
                    for i, j in GC.TERMS6 if (i, j) != (0, 0)]
        variants.append(("third plane never written", dict(planes=2)))
        for name, kw in variants:
            got = GC.split_model(c.a, c.b, **kw)
            m = GC.measure(got, ref, side, shape[2])
            assert GC.check(got, c.a, c.b, side), name
            assert 2 * m["over"] >= m["count"], f"{shape} side {side} {name}: {m['over']} of {m['count']}"


@pytest.mark.parametrize("shape", SHAPES)
def test_term_lost_in_one_chunk_or_k_group_is_flagged(cases, shape):
    K = shape[2]
    k = torch.arange(K)
    masks = {"last chunk": k < (K - 1) // 16 * 16}
    if K > 16:
        masks["k group 1 of 2"] = (k // 16) % 2 == 0
    for side in GC.SIDES:
        if not _covers(*shape, side):
            continue
        c = cases[shape, side]
        for term in GC.SECOND_ORDER:
            for name, keep in masks.items():
                got = GC.split_model(c.a, c.b, kmask={term: keep})
                bad = GC.check(got, c.a, c.b, side)
                assert bad, f"{shape} side {side}: a{term[0]}b{term[1]} lost in the {name} passes"
                # and the worst element lies at a k where the term was dropped
                m = GC.measure(got, GC.reference(c.a, c.b), side, K)
                assert not keep[m["k"]]


def test_rows_cover_every_k():
    for M, N, K in GC.FWD_CASES + GC.DX_CASES + GC.SPLITK_CASES:
        for side in GC.SIDES:
            assert _covers(M, N, K, side)
            assert sorted(set(_case(M, N, K, side).kidx.tolist())) == list(range(K))
    covered = set()
    for R, M, N, S in GC.WG_CASES:
        sides = [s for s in GC.SIDES if _covers(M, N, R, s)]
        assert sides, (R, M, N)
        for side in sides:
            assert sorted(set(_case(M, N, R, side).kidx.tolist())) == list(range(R))
            covered.add(side)
    assert covered == set(GC.SIDES)
    for s in SHAPES:
        for side in GC.SIDES:
            c = _case(*s, side)
            hot = c.a if side == "A" else c.b
            assert ((hot != 0).sum(1) == 1).all()
            assert (hot[torch.arange(hot.shape[0]), c.kidx] != 0).all()
            v = hot[torch.arange(hot.shape[0]), c.kidx]
            _, v1, v2 = GC.split(v)
            assert (v1.abs() >= 2.0 ** -11 * v.abs()).all() and (v2.abs() >= 2.0 ** -20 * v.abs()).all()
            dense = c.b if side == "A" else c.a
            # the lowest significand bit is set: the value needs all 24 bits, and the planes hold them
            assert ((dense.view(torch.int32) & 1) == 1).all()
            assert torch.equal(sum(p.double() for p in GC.split(dense)), dense.double())


def test_splitk_cases_cut_inside_a_chunk_pair_and_end_short():
    for S in GC.SPLITK_S:
        hit = 0
        for M, N, K in GC.SPLITK_CASES:
            ks = GC.kslice(K, S)
            if (S - 1) * ks >= K:
                continue  # refused by the entry: a slice would be empty
            last = K - (S - 1) * ks
            hit += (ks // 16) % 2 == 1 and last < ks and last % 16 != 0
        assert hit >= 1, S
    # the weight-gradient cases: a short last slice, empty slices (S = 40), one slice
    assert [GC.kslice(R, S) for R, _, _, S in GC.WG_CASES] == [256, 96, 16, 64]


def test_sliced_reference_and_exact_zeros():
    c = _case(40, 36, 33, "A")
    ks = GC.kslice(33, 3)
    ref = GC.reference(c.a, c.b, 3, ks)
    assert torch.equal(ref.sum(0), GC.reference(c.a, c.b))
    assert ((ref != 0).sum(0) == 1).all()
    got = torch.stack([GC.split_model(c.a[:, s * ks:(s + 1) * ks], c.b[:, s * ks:(s + 1) * ks]) for s in range(3)])
    assert GC.check(got, c.a, c.b, "A", ref=ref) == []
    leak = got.clone()
    leak[1, 0, 0] = 1e-30  # row 0 has k = 0: slice 1 must hold an exact 0 there
    assert ref[1, 0, 0] == 0 and len(GC.check(leak, c.a, c.b, "A", ref=ref)) == 1
    poison = got.clone()
    poison[0, 3, 5] = float("nan")
    assert GC.check(poison, c.a, c.b, "A", ref=ref)


def test_one_ulp_bound_of_a_single_f32_product():
    c = _case(260, 224, 219, "B")
    ref = GC.reference(c.a, c.b)
    got = ref.float()  # one rounding to nearest
    assert GC.check(got, c.a, c.b, "B", bound=GC.HALF_ULP) == []
    up = torch.nextafter(got, torch.full_like(got, float("inf")))
    dn = torch.nextafter(got, torch.full_like(got, float("-inf")))
    toward = torch.where((up.double() - ref).abs() < (dn.double() - ref).abs(), up, dn)  # the other neighbour
    toward = torch.where(got.double() == ref, got, toward)
    assert GC.check(toward, c.a, c.b, "B", bound=GC.ULP) == []
    assert GC.check(toward, c.a, c.b, "B", bound=GC.HALF_ULP)


@pytest.mark.parametrize("align", GC.ALIGNS)
def test_embedded_operand_is_surrounded_by_nan(align):
    x = GC.one_hot(37, 33, 5, "A").b
    table, view = GC.embed(x, align)
    assert torch.equal(view, x) and view.shape == x.shape
    mask = torch.ones_like(table, dtype=torch.bool)
    top = (view.data_ptr() - table.data_ptr()) // 4 // table.stride(0)
    left = (view.data_ptr() - table.data_ptr()) // 4 % table.stride(0)
    mask[top:top + 37, left:left + 33] = False
    assert top >= 1 and left >= 3 and table.shape[0] - top - 37 >= 1 and table.shape[1] - left - 33 >= 1
    assert torch.isnan(table[mask]).all() and not torch.isnan(table[~mask]).any()
    if align == 16:
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0
    else:
        assert view.stride(0) % 4 != 0 and left % 4 != 0
