"""The host reference of the fit tail (tests/fit_tail_ref.py) checked against itself and against planted faults - no GPU.

What tests/test_gpu_fit_tail.py relies on: the exact integer sums and the longdouble sums agree; the layout helper and the padded
traversal reproduce them in any spot order; and each fault a fit-tail kernel can plausibly have - a spot dropped, spot n - 1 counted
twice (the lanes past n mirror it), a neighbour missing, a non-zero pad row, a block of XtX above the diagonal weighted 1 instead of
2 - changes an integer and trips the comparator on the test's own inputs.
"""
import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref as ref


def _case(n=200, K=9, seed=3):
    coords = ref.tie_free_coords(n, 2, seed)
    A = orc.knn_graph_kdtree(coords, 6)
    beta, H, XtX = ref.integer_problem(n, K, seed + 1)
    return A, beta, H, XtX


def test_exact_sums_against_dense_algebra():
    A, beta, H, XtX = _case()
    L = np.diag(np.asarray(A.sum(1)).ravel()) - A.toarray()
    want = (int(round((beta * H.T).sum())), int(round(np.trace(beta @ XtX @ beta.T))), int(round(np.trace(beta.T @ L @ beta))),
            int(round(np.abs(beta).sum())))
    assert ref.four_sums_exact(A, beta, H, XtX) == want
    assert beta.min() < 0 and want[3] != int(round(beta.sum()))        # the fabs of the l1 term matters on these inputs


def test_longdouble_sums_agree_with_the_exact_ones():
    A, beta, H, XtX = _case()
    exact = ref.four_sums_exact(A, beta, H, XtX)
    sums, mags = ref.four_sums_longdouble(A, beta, H, XtX)
    for t in range(4):
        assert int(sums[t]) == exact[t] and sums[t] == exact[t], ref.TERMS[t]
        assert mags[t] >= abs(sums[t])
    ref.assert_sums_exact([float(x) for x in exact], exact, "self")
    ref.assert_sums_close([float(x) for x in exact], sums, mags, (1, 1, 1, 1), "self")


def test_objective_scalar_matches_the_oracle():
    A, beta, H, XtX = _case(150, 5, 8)
    want = orc.objective(beta, H, XtX, 1234.0, A, 0.25, 0.125)
    got = ref.objective_from_sums(ref.four_sums_exact(A, beta, H, XtX), 1234.0, 0.25, 0.125)
    assert got == want                                                 # integers and dyadic weights: exact on both sides


def test_quad_by_blocks_is_the_full_quadratic_term():
    A, beta, H, XtX = _case(50, 150, 5)
    full = ref.four_sums_exact(A, beta, H, XtX, quad_block=1024)
    assert ref.four_sums_exact(A, beta, H, XtX, quad_block=64) == full
    assert ref.four_sums_exact(A, beta, H, XtX, quad_block=16) == full


@pytest.mark.parametrize("shuffle", [False, True])
def test_layout_and_padded_traversal_reproduce_the_sums(shuffle):
    A, beta, H, XtX = _case()
    n = beta.shape[0]
    perm = np.random.RandomState(0).permutation(n) if shuffle else None
    P, Hp = ref.to_planes(beta, perm), ref.h_to_planes(H, perm)
    assert P.shape == (beta.shape[1], ref.round_up(n + 1, 64)) and not P[:, n:].any() and np.isnan(Hp[:, n:]).all()
    lists, deg = ref.padded_lists(A, perm)
    assert (lists == n).sum() == lists.size - A.nnz                    # rows shorter than the width are padded with n
    assert ref.four_sums_planes(P, Hp, XtX, lists, deg, n) == ref.four_sums_exact(A, beta, H, XtX)


# ------------------------------------------------------------------------------------------------ planted faults
def _trips(exact, wrong, term):
    assert wrong != exact and wrong[term] != exact[term]
    with pytest.raises(AssertionError, match="objective sums off"):
        ref.assert_sums_exact([float(x) for x in wrong], exact, "planted")


def test_comparator_fails_on_one_spot_dropped():
    A, beta, H, XtX = _case()
    n = beta.shape[0]
    exact = ref.four_sums_exact(A, beta, H, XtX)
    for drop in (0, 63, 64, n - 1):
        wrong = ref.four_sums_exact(A, beta, H, XtX, spots=np.delete(np.arange(n), drop))
        _trips(exact, wrong, 3)                                        # every row has a non-zero entry: l1 moves at least
    assert np.abs(beta).sum(1).min() > 0


def test_comparator_fails_on_last_spot_counted_twice():
    A, beta, H, XtX = _case()
    exact = ref.four_sums_exact(A, beta, H, XtX)
    _trips(exact, ref.four_sums_exact(A, beta, H, XtX, count_twice=beta.shape[0] - 1), 3)


def test_comparator_fails_on_one_neighbour_missing():
    A, beta, H, XtX = _case()
    exact = ref.four_sums_exact(A, beta, H, XtX)
    A = sparse.csr_matrix(A)
    hit = 0
    for i in (0, 17, beta.shape[0] - 1):
        for j in A.indices[A.indptr[i]:A.indptr[i + 1]]:
            if beta[i] @ beta[j] != 0 or (beta[i] ** 2).sum() != 0:
                A2 = A.tolil()
                A2[i, j] = 0                                           # one directed entry: spot i loses neighbour j
                A2 = A2.tocsr()
                A2.eliminate_zeros()
                wrong = ref.four_sums_exact(A2, beta, H, XtX)
                assert wrong[:2] == exact[:2] and wrong[3] == exact[3]  # only the smoothness term sees the graph
                if wrong[2] != exact[2]:
                    _trips(exact, wrong, 2)
                    hit += 1
                break
    assert hit >= 2


def test_comparator_fails_on_non_zero_pad_row():
    A, beta, H, XtX = _case()
    n = beta.shape[0]
    perm = np.random.RandomState(1).permutation(n)
    exact = ref.four_sums_exact(A, beta, H, XtX)
    lists, deg = ref.padded_lists(A, perm)
    assert (lists == n).any()                                          # some row is shorter than the width: the pad row is read
    P = ref.to_planes(beta, perm, pad_row=1.0)
    wrong = ref.four_sums_planes(P, ref.h_to_planes(H, perm), XtX, lists, deg, n)
    assert wrong[:2] == exact[:2] and wrong[3] == exact[3]
    _trips(exact, wrong, 2)


def test_comparator_fails_on_upper_block_weighted_once():
    A, beta, H, XtX = _case(50, 150, 5)
    exact = ref.four_sums_exact(A, beta, H, XtX)
    _trips(exact, ref.four_sums_exact(A, beta, H, XtX, quad_upper_weight=1), 1)
    with pytest.raises(AssertionError, match="quad"):
        ref.assert_sums_exact([float(x) for x in ref.four_sums_exact(A, beta, H, XtX, quad_upper_weight=1)], exact)


def test_rounding_comparator_fails_beyond_its_bound():
    A, _, _, _ = _case()
    beta, H, XtX = ref.real_problem(200, 9, 4)
    sums, mags = ref.four_sums_longdouble(A, beta, H, XtX)
    got = [float(s) for s in sums]
    ref.assert_sums_close(got, sums, mags, (2, 2, 2, 2), "self")
    got[2] += 1e-9 * float(mags[2])
    with pytest.raises(AssertionError, match="spat"):
        ref.assert_sums_close(got, sums, mags, (1000, 1000, 1000, 1000), "planted")
    got[2] = float("nan")
    with pytest.raises(AssertionError, match="spat"):
        ref.assert_sums_close(got, sums, mags, (1000, 1000, 1000, 1000), "planted NaN")


# ------------------------------------------------------------------------------------------------ export
def test_export_ref_follows_the_reference_rule():
    K = 5
    kinds = {i: k for i, k in enumerate(ref.EXPORT_KINDS)}
    B = ref.export_rows(12, K, kinds, 2)
    B[7, 2] = np.nan
    beta_out, prop = ref.export_ref(B)
    with np.errstate(invalid="ignore"):
        want = orc.normalize_proportions(B.copy())
    ref.assert_same_bits(prop, want, "prop_out")
    ref.assert_same_bits(beta_out, B, "beta_out")
    assert (prop[0] == 1 / K).all() and (prop[1] == 1 / K).all() and np.signbit(beta_out[1]).all()
    assert ref.row_sums(B)[2] == 5e-11 and prop[2, 0] == 2.5e-11 / 1e-10 and prop[2].sum() == pytest.approx(0.5)
    assert ref.row_sums(B)[3] < 0 and (prop[3] == B[3] / 1e-10).all()
    assert B[4].any() and ref.row_sums(B)[4] == 0 and (prop[4] == 1 / K).all()
    assert np.isnan(prop[7]).all() and np.isfinite(prop[np.arange(12) != 7]).all()
    assert np.allclose(prop[8:].sum(1), 1.0)
    lp = ref.export_ref_longdouble(np.where(np.isnan(B), 1.0, B))
    ok = np.arange(12) != 7
    assert np.allclose(np.asarray(lp, dtype=np.float64)[ok], prop[ok], rtol=1e-15, atol=0)


def test_export_comparator_sees_sign_of_zero_and_one_entry():
    B = ref.export_rows(70, 3, {5: "negzero"}, 1)
    beta_out, prop = ref.export_ref(B)
    ref.assert_same_bits(beta_out, B, "beta_out")
    with pytest.raises(AssertionError, match="first row 5"):
        ref.assert_same_bits(np.where(B == 0, 0.0, B), B, "beta_out")   # -0.0 exported as +0.0
    p2 = prop.copy()
    p2[69, 2] = np.nextafter(p2[69, 2], 1.0)
    with pytest.raises(AssertionError, match="first row 69.*column 2"):
        ref.assert_same_bits(p2, prop, "prop_out")
    # fmax(sum, 1e-10) instead of np.maximum: the finite entries of a row that holds a NaN come out as v / 1e-10
    B[9, 1] = np.nan
    _, want = ref.export_ref(B)
    wrong = want.copy()
    wrong[9] = B[9] / 1e-10
    with pytest.raises(AssertionError, match="first row 9"):
        ref.assert_same_bits(wrong, want, "prop_out")


# ------------------------------------------------------------------------------------------------ dispatch
def test_tiled_objective_dispatches_every_sweep_part():
    """The tiled sweep's instantiations are compiled in parts (PARTS of csrc/Makefile, one bcd_sweep_dispatch_part<p> each).  The
    objective pass must try every part the sweep tries: a part left out sends its cell-type counts through the generic kernel - same
    sums, so only the route shows it (K = 60..64 went that way after the parts were rebalanced into ten)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flashdeconv_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        parts = re.search(r"^PARTS\s*=\s*(.+)$", f.read(), re.M).group(1).split()
    ids = sorted(int(p.split(":")[0]) for p in parts)
    covered = set()
    for p in parts:
        _, lo, hi, step = (int(x) for x in p.split(":"))
        covered.update(range(lo, hi + 1, step))
    assert covered == set(range(1, 65)) | {72, 80, 88, 96}
    with open(os.path.join(csrc, "bcd_kernels.cpp")) as f:
        src = f.read()

    def tried(func):
        body = src[src.index(func):]
        body = body[:body.index("\n}\n")]
        return sorted(int(m) for m in re.findall(r"bcd_sweep_dispatch_part(\d+)\(a, st\)", body))

    assert tried("int launch_bcd_sweep(") == ids
    assert tried("int launch_bcd_objective_tiled(") == ids
