"""CPU checks of tests/sparsify_cases.py: every grid on which the device assembly is judged must be a fair question, and the
device algorithm itself (Gram matrix, Hermitian eigensolve, one first-order correction: sparsify_ref.gram_refine, numpy
double) must reach the accuracy of the SVD reference there.  No GPU.

Input conditions, per class: sigma_-2 / sigma_min >= 1.2 and sigma_min / sigma_max >= 1e-5.  The smallest singular vector of
np.linalg.svd is only trustworthy under them; a case that breaks them is a bad case, not a loose bound.

With e(v) the phase-aligned 2-norm distance to the SVD vector and b_c = eps sigma_max / (sigma_-2 - sigma_min):
    e(corrected) <= 2 b_c             in every class of every case (measured: <= 0.681 b_c, at trap-21x41; the table is in
                                      DESIGN.md);
    e(uncorrected) > 8 b_c            in at least one class of each low-k case, so that the bound of
                                      tests/test_gpu_sparsify_shapes.py can fail a build without the refinement.
sparsify_cases.MARGIN, the factor of the device bound, is 4 x the largest e(corrected) / b_c over CASES, 4 x 0.681; this file
asserts that CASES stays under MARGIN / 4 (the two literal symbols of the evenness tests measure 0.83 and 0.74 and are held
to 2 b_c only; they have an input condition of their own, cancel_c <= 2, see sparsify_cases.SELF)."""
import numpy as np
import pytest

import sparsify_cases as sc
import sparsify_ref as ref

MIN_GAP, MIN_COND = 1.2, 1e-5


def _judge(r, what, in_table=True):
    gap, cond = sc.conditions(r)
    e_corr, e_unc, b = r["refine"].T
    print(f"{what}: sigma_-2/sigma_min >= {gap:.3f}, sigma_min/sigma_max >= {cond:.2e}, e(corrected)/b <= {(e_corr / b).max():.3f}, "
          f"e(uncorrected)/b <= {(e_unc / b).max():.1f}, e(uncorrected) <= {e_unc.max():.2e}")
    assert gap >= MIN_GAP and cond >= MIN_COND, (what, gap, cond)
    assert np.all(e_corr <= 2.0 * b), (what, (e_corr / b).max())
    assert not in_table or (e_corr / b).max() <= sc.MARGIN / 4.0, (what, (e_corr / b).max())
    return e_unc / b


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_case_is_well_posed_and_the_algorithm_reaches_the_reference(case):
    unc = _judge(sc.reference(case), sc.case_id(case))
    if case.kind == "lowk":
        assert unc.max() > 8.0, (sc.case_id(case), unc.max())


@pytest.mark.parametrize("dims", sorted(sc.LITERAL), ids=lambda d: "x".join(map(str, d)))
def test_literal_symbols_are_well_posed_and_what_they_claim(dims):
    r = sc.literal_reference(dims)
    _judge(r, f"literal {dims}", in_table=False)
    # the AG row must not cancel (sparsify_cases.SELF): an error of the vector grows by this factor in a_c G[S_c, S_c]
    print(f"literal {dims}: |G[S,S]| / |a G[S,S]| <= {r['cancel'].max():.2f}")
    assert r["cancel"].max() <= sc.MAX_CANCEL, r["cancel"]
    flip = lambda G, axes: np.roll(np.flip(G, axis=axes), 1, axis=axes)   # noqa: E731
    axes = tuple(range(len(dims)))
    scale = lambda G: np.abs(G).max()                       # noqa: E731
    G = sc.literal_symbol(dims, "none")
    assert np.abs(G - flip(G, axes)).max() > 0.1 * scale(G)
    G = sc.literal_symbol(dims, "point")
    assert np.abs(G - flip(G, axes)).max() <= 1e-15 * scale(G)
    for ax in axes:                                         # symmetric as a matrix, but even along no single axis
        assert np.abs(G - flip(G, (ax,))).max() > 0.1 * scale(G), ax
    G = sc.literal_symbol(dims, "axes")
    for ax in axes:
        assert np.abs(G - flip(G, (ax,))).max() <= 1e-15 * scale(G), ax


def test_gram_refine_on_a_matrix_with_known_singular_vectors():
    # Gs = U diag(s) V^H with singular values down to 1e-5: the uncorrected Gram vector loses what the squared condition
    # number costs, the corrected one is back at the reference's own accuracy
    rng = np.random.default_rng(3)
    ns, N = 9, 400
    U, _ = np.linalg.qr(rng.standard_normal((ns, ns)) + 1j * rng.standard_normal((ns, ns)))
    V, _ = np.linalg.qr(rng.standard_normal((N, ns)) + 1j * rng.standard_normal((N, ns)))
    s = np.array([1.0, 0.5, 0.2, 1e-1, 1e-2, 1e-3, 1e-4, 2e-5, 1e-5])
    Gs = (U * s) @ V.conj().T
    corrected, uncorrected = ref.gram_refine(Gs)
    b = sc.EPS * s[0] / (s[-2] - s[-1])
    assert ref.phase_distance(corrected, U[:, -1]) <= 4.0 * b
    assert ref.phase_distance(uncorrected, U[:, -1]) > 100.0 * b


def test_tile_counts_are_what_the_table_says():
    t = {sc.case_id(c): sc.tiles(c) for c in sc.CASES}
    assert t["trap-127x129"] == (256, 1, 63) and t["trap-129x127"] == (256, 1, 63)
    assert t["trap-129x129"] == (261, 2, 1) and t["trap-257x65"] == (262, 2, 1)
    assert t["trap-183x181"] == (518, 3, 35)
    assert t["gv3-4x4x4"] == (1, 1, 64) and t["trap-5x5"] == (1, 1, 25)
    assert t["gv3-26x26x26"] == (275, 2, 40) and t["gv3-16x32x34"] == (272, 2, 64) and t["gv3-32x32x34"] == (544, 3, 64)
    assert len({sc.case_id(c) for c in sc.CASES}) == len(sc.CASES)
