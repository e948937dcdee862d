"""CPU tests of the host restatement of partial pivoting (tests/blocktri_pivot_ref.py) and of the inputs that the GPU
tests of tests/test_gpu_blocktri_pivot.py are built on.

b = 2 is the one permuted shape on which Gauss-Jordan without pivoting does not break down: `synth` stores both columns of
a 2 x 2 block with random values, so the pivot that the interchange brings up is an off-diagonal entry of modulus O(1)
against a diagonal of a few units (ratio 0.1 to 0.5), whatever the seed; a ratio below 1e-8 would take ~1e8 seeds.  For
that shape the test asserts what does hold: every Pi_k is the interchange, the rule takes row 1 first in every block,
and the pivot without pivoting is the smaller candidate.  From b = 31 on the patterns are sparse and a permuted block
has a structural zero on its diagonal: the ratio is exactly 0."""
import numpy as np
import pytest

import blocktri_ref as bt
import blocktri_cases as bc
import blocktri_pivot_ref as pv

shapes = pytest.mark.parametrize("shape", pv.PERMUTED_SHAPES, ids=bc.shape_id)


@pytest.mark.parametrize("b", [1, 2, 7, 33, 70])
def test_inverse_against_numpy(b):
    rng = np.random.default_rng(b)
    A = rng.standard_normal((b, b)) + 1j * rng.standard_normal((b, b))
    inv, perm, ratio = pv.gauss_jordan_partial(A)
    ref = np.linalg.inv(A)
    err = np.linalg.norm(inv - ref) / np.linalg.norm(ref)
    print(f"b = {b}: gauss_jordan_partial vs np.linalg.inv {err:.2e}, min ratio {ratio:.3e}")
    assert err <= 1e-12
    assert np.array_equal(np.sort(perm), np.arange(b)) and 0.0 < ratio <= 1.0 + 1e-12      # (|piv| and max|A| round on their own)


def test_rule():
    # the largest modulus wins, the lowest row on a tie, and only rows that have not been pivot rows are candidates
    A = np.array([[1.0, 2.0, 0.0], [-2.0j, 1.0, 1.0], [2.0, 0.0, 5.0]], dtype=np.complex128)
    inv, perm, ratio = pv.gauss_jordan_partial(A)
    assert perm[0] == 1                                    # |-2i| = |2|: row 1 before row 2
    assert np.linalg.norm(inv @ A - np.eye(3)) <= 1e-14
    # a zero leading pivot is no obstacle
    P = np.eye(5)[[3, 0, 4, 1, 2]]
    inv, perm, ratio = pv.gauss_jordan_partial(P)
    assert np.array_equal(inv, P.T) and np.array_equal(perm, [1, 3, 4, 0, 2]) and ratio == 1.0
    # the planted 2 x 2: the interchange, and the ratio 1 instead of eps
    inv, perm, ratio = pv.gauss_jordan_partial(np.array([[1e-9, 1.0], [1.0, 1e-9]]))
    assert np.array_equal(perm, [1, 0]) and ratio == 1.0
    # singular under pivoting
    assert pv.gauss_jordan_partial(np.ones((3, 3)))[2] < 1e-8


@shapes
def test_permuted_pair(shape):
    b, K, _ = shape
    Mp, Ap, perms, Msp, As = pv.case(shape)
    # one sorted pattern inside the three block diagonals
    assert np.array_equal(Mp.indices, Ap.indices) and np.array_equal(Mp.indptr, Ap.indptr)
    assert bt.in_band(Mp.indptr, Mp.indices, K) and Mp.has_sorted_indices
    assert all(np.all(np.diff(Mp.indices[Mp.indptr[r]:Mp.indptr[r + 1]]) > 0) for r in range(b * K))
    assert Mp.nnz == Msp.nnz
    # S'_k = Pi_k S_k
    S, Sp = bc.schur_blocks(Msp, K), bc.schur_blocks(Mp, K)
    for k in range(K):
        err = np.abs(Sp[k] - S[k][perms[k]]).max() / np.abs(S[k]).max()
        assert err <= 1e-13, f"block {k}: {err}"
    # the restatement on the permuted blocks: S_k^{-1} Pi_k^T, pivots far from the threshold
    for k in range(K if b <= 257 else 0):
        inv, perm, ratio = pv.gauss_jordan_partial(Sp[k])
        ref = np.linalg.inv(S[k])[:, perms[k]]
        assert np.linalg.norm(inv - ref) <= 1e-12 * np.linalg.norm(ref)
        assert np.array_equal(np.sort(perm), np.arange(b)) and ratio >= 1e-2
        perm_lu, ratio_lu = pv.pivots_partial(Sp[k])
        assert np.array_equal(perm_lu, perm) and abs(ratio_lu - ratio) <= 1e-12 * ratio


@shapes
def test_permuted_pair_needs_pivoting(shape):
    b, K, _ = shape
    Mp, _, perms, Msp, _ = pv.case(shape)
    Sp = bc.schur_blocks(Mp, K)
    m = min(b, 64)                                         # the first m pivots are those of the leading m x m block
    with np.errstate(all="ignore"):
        ratios = [bt.gauss_jordan_nopivot(S[:m, :m])[1] for S in Sp]
    print(f"{bc.shape_id(shape)}: |pivot| / max|S_k| of Gauss-Jordan without pivoting per block {ratios}")
    if b == 2:                                             # (module docstring)
        for k in range(K):
            assert np.array_equal(perms[k], [1, 0])
            _, perm, ratio = pv.gauss_jordan_partial(Sp[k])
            assert perm[0] == 1 and abs(Sp[k][0, 0]) < abs(Sp[k][1, 0]) and ratios[k] < ratio
        return
    assert min(ratios) < 1e-8


def test_planted():
    b, K = pv.PLANT_B, pv.PLANT_K
    for eps in (1e-9, 0.0):
        Msp, As = pv.planted(eps)
        assert np.array_equal(Msp.indices, As.indices) and bt.in_band(Msp.indptr, Msp.indices, K)
        S = bc.schur_blocks(Msp, K)
        assert np.array_equal(S[1], Msp[b:2 * b, b:2 * b].toarray()) and np.abs(S[1]).max() == pv.PLANT_SMAX
        with np.errstate(all="ignore"):
            assert bt.gauss_jordan_nopivot(S[1])[1] <= 1e-9
        want = np.arange(b)
        want[[45, 46]] = [46, 45]
        for k in range(K):
            inv, perm, ratio = pv.gauss_jordan_partial(S[k])
            assert ratio >= 1e-2
            if k == 1:
                assert np.array_equal(perm, want) and ratio == 1.0


def test_tie_and_singular_inputs():
    Msp, As = pv.tie_pair()
    assert np.array_equal(Msp.indices, As.indices)
    S = Msp.toarray()
    first = S[:, 0]
    assert np.all(first.real * first.real + first.imag * first.imag == 1.0)
    inv, perm, ratio = pv.gauss_jordan_partial(S)
    assert perm[0] == 0 and ratio >= 1e-2 and np.linalg.norm(inv @ S - np.eye(40)) <= 1e-12
    Msp, As = pv.singular_pair()
    assert np.array_equal(Msp.indices, As.indices) and bt.in_band(Msp.indptr, Msp.indices, 2)
    S = bc.schur_blocks(Msp, 2)
    assert np.array_equal(S[1][5], S[1][9])
    assert pv.gauss_jordan_partial(S[0])[2] >= 1e-2 and pv.gauss_jordan_partial(S[1])[2] < 1e-8
