"""-m gpu tests of the cell-type expression statistics (csrc/expression_kernels.cpp: fdx_weighted_gene_sums_dev / _csr_dev and
fdx_nnls_gram_dev; utils.expression; FlashDeconv.get_celltype_expression; tl.deconvolve(celltype_expression=True)).

Reference: tests/expression_ref.py (the NumPy definition; checked against scipy in tests/test_expression_host.py, which also
asserts the two conditions used here: the exact cases are exactly representable in any order, and every gene of every generic
case converges in the reference).

Exact cases (weights in sixteenths, counts 0 .. 7) must EQUAL the reference on every route: no tolerance.  The generic solves are
held to the KKT bound of expression_ref.kkt with a factor 2 (the device keeps the running gradient, which reorders the rounding),
and to the measured bounds below.
"""
import numpy as np
import pytest

import datagen
import expression_ref as er
from conftest import load_golden

pytestmark = pytest.mark.gpu

SEG = 2048            # FDX_EXPRESSION_SEGMENT_ROWS: the kernel's stripe edge
ROUTES = ["host_f32", "host_f64", "dev_f32", "dev_f64", "dev_strided", "csr_scipy", "csr_cuda", "csr_unsorted", "csr_holes", "host_int"]

# Measured on the MI355X against the reference ("Cell-type expression"): the bounds are 4x the measurements.
#   max over the genes of max_k |S_dev - S_ref| / max_k S_ref, worst case (K = 130):     tol 1e-6: 5.9e-14     tol 1e-10: 5.7e-14
#   max |rss_dev - rss_ref| / (K eps (q + 2 |s|.|b| + |s|'|A||s|)), worst case (K = 5):    c = 0.15
# (the device and the reference stopped after the same number of sweeps in every gene of every case)
EXPRESSION_BOUND = {1e-6: 4 * 5.9e-14, 1e-10: 4 * 5.7e-14}
RSS_C_BOUND = 4 * 0.15


def _route_Y(Y, route):
    """The container of `route` holding the integer-valued float matrix Y."""
    import torch
    from scipy import sparse
    if route == "host_f32":
        return Y.astype(np.float32)
    if route == "host_f64":
        return Y.astype(np.float64)
    if route == "host_int":
        return Y.astype(np.int32)
    if route == "dev_f32":
        return torch.as_tensor(Y.astype(np.float32)).cuda()
    if route == "dev_f64":
        return torch.as_tensor(Y.astype(np.float64)).cuda()
    if route == "dev_strided":                       # a column window of a wider matrix: row stride G + 7
        wide = torch.full((Y.shape[0], Y.shape[1] + 7), 99.0, dtype=torch.float32, device="cuda")
        wide[:, 3:3 + Y.shape[1]] = torch.as_tensor(Y.astype(np.float32)).cuda()
        return wide[:, 3:3 + Y.shape[1]]
    if route == "csr_scipy":
        return sparse.csr_matrix(Y.astype(np.float32))
    if route == "csr_cuda":
        m = sparse.csr_matrix(Y.astype(np.float64))
        return torch.sparse_csr_tensor(torch.as_tensor(m.indptr.astype(np.int64)), torch.as_tensor(m.indices.astype(np.int32)),
                                       torch.as_tensor(m.data), size=m.shape).cuda()
    if route == "csr_unsorted":                      # every row's columns reversed
        m = sparse.csr_matrix(Y.astype(np.float32))
        idx, dat = m.indices.copy(), m.data.copy()
        for i in range(m.shape[0]):
            a, b = m.indptr[i], m.indptr[i + 1]
            idx[a:b], dat[a:b] = idx[a:b][::-1], dat[a:b][::-1]
        u = sparse.csr_matrix((dat, idx, m.indptr), shape=m.shape)
        assert not u.has_sorted_indices or np.all(np.diff(m.indptr) < 2)
        return u
    raise ValueError(route)


def _exact_case(n, G, K, groups, route, seed=0):
    W = er.dyadic_weights(n, K, seed)
    Y = er.integer_counts(n, G, seed, density=0.3 if route.startswith("csr") else 1.0, dtype=np.float64)
    if route == "csr_holes":                         # empty rows and an all-zero gene
        Y[::3] = 0.0
        Y[:, G // 2] = 0.0
    g, C = er.group_labels(n, groups, seed)
    return Y, W, g, C


def _sums_cases():
    ns = [1, 2, 63, 64, 65, 257, 1000, SEG - 1, SEG, SEG + 1, 2 * SEG + 1]
    Gs = [1, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513]        # 256: a wave group's genes, 512: a workgroup's
    Ks = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 130]
    kinds = ["none", "three", "empty", "single"]
    cases, i = [], 0
    for n in ns:                                     # every n, crossed with a few of the others
        for t in range(2):
            cases.append((n, Gs[(i + 3 * t) % len(Gs)], Ks[(2 * i + 5 * t) % len(Ks)], kinds[(i + t) % 4] if n >= 64 else "none",
                          ROUTES[(i + 4 * t) % len(ROUTES)]))
            i += 1
    for G in Gs:
        for t in range(2):
            cases.append((ns[4 + (i % 5)], G, Ks[(3 * i + t) % len(Ks)], kinds[(i + 2 * t) % 4], ROUTES[(i + 3 * t + 1) % len(ROUTES)]))
            i += 1
    for K in Ks:
        for t in range(2):
            cases.append((ns[4 + ((i + t) % 4)], Gs[(i + 5 * t) % len(Gs)], K, kinds[(i + t) % 4], ROUTES[(i + 5 * t) % len(ROUTES)]))
            i += 1
    for r, route in enumerate(ROUTES):               # every route with groups and more than one segment
        cases.append((SEG + 65, 65, 33, kinds[1 + r % 3], route))
    for G in (255, 256, 257, 511, 512, 513):         # the dense kernel's gene edges on dense routes, the last type chunk 32 and 16 wide
        cases += [(257, G, 33, "three", "dev_f32"), (65, G, 17, "none", "host_f64")]
    return sorted(set(cases))


@pytest.mark.parametrize("n,G,K,groups,route", _sums_cases())
def test_sums_equal_the_reference_exactly(n, G, K, groups, route):
    from flashdeconv_amd.utils.expression import weighted_gene_sums
    Y, W, g, C = _exact_case(n, G, K, groups, route)
    A, B, q, u, n_rows = er.sums(Y, W, g, C)
    got = weighted_gene_sums(_route_Y(Y, "csr_scipy" if route == "csr_holes" else route), W, groups=g, n_groups=C)
    for key, want in (("A", A), ("B", B), ("q", q), ("u", u), ("n_rows", n_rows)):
        want = want[0] if g is None else want
        have = np.asarray(got[key])
        assert have.shape == np.shape(want), (key, have.shape)
        assert np.array_equal(have, want), (key, float(np.abs(have - want).max()))


def test_sums_from_device_weights_and_labels_stay_on_the_device():
    import torch
    from flashdeconv_amd.utils.expression import weighted_gene_sums
    Y, W, g, C = _exact_case(SEG + 300, 70, 20, "three", "dev_f32", seed=4)
    want = er.sums(Y, W, g, C)
    wide = torch.zeros((W.shape[0], 29), dtype=torch.float64, device="cuda")
    wide[:, 5:25] = torch.as_tensor(W).cuda()
    got = weighted_gene_sums(_route_Y(Y, "dev_f32"), wide[:, 5:25], groups=torch.as_tensor(g).cuda(), n_groups=C)
    for key, w in zip(("A", "B", "q", "u"), want):
        assert got[key].is_cuda and np.array_equal(got[key].cpu().numpy(), w), key
    assert np.array_equal(got["n_rows"], want[4])


@pytest.mark.parametrize("route", ["host_f32", "dev_f64", "csr_scipy", "csr_cuda"])
def test_two_calls_and_another_stripe_count_return_the_same_bits(route, monkeypatch):
    """Generic (inexact) data over three segments per group at the most: a second call, and calls whose workgroups take 2 or 5
    segments each (FDX_EXPR_STRIPE_SEGMENTS), return the bits of the first."""
    from flashdeconv_amd.utils.expression import weighted_gene_sums
    rs = np.random.RandomState(5)
    n, G, K = 3 * SEG + 77, 130, 33
    W = rs.dirichlet(np.full(K, 0.5), size=n)
    Y = rs.gamma(0.5, 3.0, size=(n, G)) * (rs.rand(n, G) < 0.4)
    g = rs.randint(-1, 2, size=n)
    Yc = _route_Y(Y, route)
    first = weighted_gene_sums(Yc, W, groups=g, n_groups=2)
    again = weighted_gene_sums(Yc, W, groups=g, n_groups=2)
    for key in ("A", "B", "q", "u"):
        assert np.array_equal(first[key], again[key]), key
    ref = er.sums(Y.astype(np.float32) if "f32" in route or route == "csr_scipy" else Y, W, g, 2)
    assert np.allclose(first["B"], ref[1], rtol=1e-12, atol=0) and np.allclose(first["A"], ref[0], rtol=1e-12, atol=0)
    for stripe in ("2", "5"):
        monkeypatch.setenv("FDX_EXPR_STRIPE_SEGMENTS", stripe)
        other = weighted_gene_sums(Yc, W, groups=g, n_groups=2)
        for key in ("A", "B", "q", "u"):
            assert np.array_equal(first[key], other[key]), (stripe, key)


@pytest.mark.parametrize("route", ["dev_f32", "csr_scipy"])
def test_sums_continue_across_a_scratch_batch(route, monkeypatch):
    """More segments than the scratch holds at once (include/fdx.h: about 1 GiB of segment sums, of round_up(K, 16) + 2 planes of
    G float64 per segment): a group whose third segment is the first of the second batch continues from what the first batch
    left, the groups after it start afresh there, and another stripe count returns the same bits.  A segment never crosses a
    group, so 1790 one-row groups make 1790 segments.  Exact data: every sum must EQUAL the reference.  The budget is no switch,
    so this cannot compare with a one-batch run of the same data: that the bits do not depend on the batch follows from the
    fold's fixed ascending order; what is shown here is that no batch is dropped, doubled or started from the wrong value."""
    from flashdeconv_amd.utils.expression import weighted_gene_sums
    K, G = 130, 513
    batch = (1 << 30) // (((K + 15) // 16 * 16 + 2) * G * 8)
    sizes = [1] * 1790 + [2 * SEG + 100, 5, 0, SEG + 1]
    first_seg = np.concatenate([[0], np.cumsum([-(-s // SEG) for s in sizes])])
    long_group = 1790
    assert batch == 1792 and first_seg[-1] > batch
    assert first_seg[long_group] < batch <= first_seg[long_group + 1] - 1
    rs = np.random.RandomState(11)
    g = rs.permutation(np.concatenate([np.repeat(np.arange(len(sizes)), sizes), np.full(7, -1)])).astype(np.int64)
    n, C = g.size, len(sizes)
    W = er.dyadic_weights(n, K, 11)
    Y = er.integer_counts(n, G, 11, density=0.3 if route.startswith("csr") else 1.0, dtype=np.float64)
    want = dict(zip(("A", "B", "q", "u", "n_rows"), er.sums(Y, W, g, C)))
    Yc = _route_Y(Y, route)
    first = weighted_gene_sums(Yc, W, groups=g, n_groups=C)
    for key in want:
        have = np.asarray(first[key])
        assert have.shape == want[key].shape, (key, have.shape)
        assert np.array_equal(have, want[key]), (key, float(np.abs(have - want[key]).max()))
    monkeypatch.setenv("FDX_EXPR_STRIPE_SEGMENTS", "5")
    other = weighted_gene_sums(Yc, W, groups=g, n_groups=C)
    for key in want:
        assert np.array_equal(np.asarray(first[key]), np.asarray(other[key])), key


# ---------------------------------------------------------------- the solve, exact
@pytest.mark.parametrize("K", [1, 5, 64, 65, 130])
def test_one_hot_weights_solve_exactly_in_two_sweeps(K):
    from flashdeconv_amd.utils.expression import celltype_expression
    n, G = 40 * K + 3, 37
    W = er.dyadic_weights(n, K, 6, one_hot=True)
    Y = 1.0 + er.integer_counts(n, G, 6, dtype=np.float64)
    out = celltype_expression(Y, W)
    A, B, _, _, _ = er.sums(Y, W)
    assert np.array_equal(out["gram"], A[0]) and np.count_nonzero(A[0] - np.diag(np.diag(A[0]))) == 0 and np.all(np.diag(A[0]) > 0)
    assert np.array_equal(out["expression"], B[0] / np.diag(A[0])[:, None])
    assert np.all(out["n_iter"] == 2) and out["converged"].all() and out["estimable"].all()
    ref = er.celltype_expression(Y, W)
    assert np.array_equal(ref["expression"], out["expression"]) and np.all(ref["n_iter"] == 2)


def test_anticorrelated_gene_and_absent_type_give_exact_zeros():
    from flashdeconv_amd.utils.expression import celltype_expression
    n, G, K = 600, 12, 4
    W = er.dyadic_weights(n, K, 7)
    Y = er.integer_counts(n, G, 7, dtype=np.float64)
    Y[:, 5] = 8.0 * W[:, 0] * (W[:, 1] == 0)         # expressed by type 0 only where type 1 is absent
    g, C = er.group_labels(n, "three", 7)
    W[g == 2, 3] = 0.0                               # type 3 absent from group 2
    ref, ref_g = er.celltype_expression(Y, W), er.celltype_expression(Y, W, g, C)
    assert ref["expression"][1, 5] == 0.0 and ref["expression"][0, 5] > 0
    out, out_g = celltype_expression(Y, W), celltype_expression(Y, W, groups=g, n_groups=C)
    assert out["expression"][1, 5] == 0.0 and out["expression"][0, 5] > 0
    assert np.array_equal(out["expression"] == 0, ref["expression"] == 0)
    assert np.all(out_g["expression"][2, 3] == 0.0) and not out_g["estimable"][2, 3]
    assert np.array_equal(out_g["estimable"], ref_g["estimable"]) and out_g["estimable"].sum() == C * K - 1
    assert np.array_equal(out_g["n_rows"], ref_g["n_rows"]) and np.array_equal(out_g["gram"], ref_g["gram"])
    assert np.array_equal(out_g["tss"], ref_g["tss"])       # exact sums, the same operations


# ---------------------------------------------------------------- the solve, generic
_GENERIC_REF = {}


def _generic(case, tol, groups=None, ridge=0.0):
    key = (case, tol, groups, ridge)
    if key not in _GENERIC_REF:
        n, G, K, seed = case
        Y, W = er.generic_case(n, G, K, seed)
        g, C = er.group_labels(n, groups, seed) if groups else (None, None)
        ref = er.celltype_expression(Y, W, g, C, ridge=ridge, max_iter=er.GENERIC_MAX_ITER, tol=tol)
        for a in [Y, W] + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _GENERIC_REF[key] = (Y, W, g, C, ref)
    return _GENERIC_REF[key]


def _check_generic(case, tol, groups=None, ridge=0.0):
    from flashdeconv_amd.utils.expression import celltype_expression, weighted_gene_sums
    Y, W, g, C, ref = _generic(case, tol, groups, ridge)
    K = W.shape[1]
    out = celltype_expression(Y, W, groups=g, n_groups=C, ridge=ridge, max_iter=er.GENERIC_MAX_ITER, tol=tol)
    sums = weighted_gene_sums(Y, W, groups=g, n_groups=C)
    assert np.array_equal(sums["A"], out["gram"])
    assert out["converged"].all() and ref["converged"].all()
    lead = (lambda a: a) if g is not None else (lambda a: a[None])
    worst_kkt = worst_diff = worst_c = worst_r2 = 0.0
    for c in range(C or 1):
        A, B, q = lead(sums["A"])[c], lead(sums["B"])[c], lead(sums["q"])[c]
        S, S_ref = lead(out["expression"])[c], lead(ref["expression"])[c]
        if ridge == 0.0:
            worst_kkt = max(worst_kkt, er.kkt_worst(A, B, S, tol))
        worst_diff = max(worst_diff, float((np.abs(S - S_ref).max(axis=0) / S_ref.max(axis=0)).max()))
        scale = K * er.EPS * er.rss_scale(A, B, q, S_ref)
        d_rss = np.abs(lead(out["rss"])[c] - lead(ref["rss"])[c])
        worst_c = max(worst_c, float((d_rss / scale).max()))
        tss = lead(ref["tss"])[c]
        assert np.array_equal(np.isnan(lead(out["r2"])[c]), tss == 0)
        ok = tss > 0
        r2_bound = RSS_C_BOUND * scale[ok] / tss[ok] + 8 * er.EPS * (1 + lead(ref["rss"])[c][ok] / tss[ok])
        worst_r2 = max(worst_r2, float((np.abs(lead(out["r2"])[c][ok] - lead(ref["r2"])[c][ok]) / r2_bound).max()))
        np.testing.assert_allclose(lead(out["tss"])[c], tss, rtol=64 * er.EPS * max(1.0, float((q / np.where(ok, tss, 1)).max())), atol=0)
    d_it = int(np.abs(out["n_iter"].astype(np.int64) - ref["n_iter"]).max())
    print(f"expression generic case={case} tol={tol:g} groups={groups} ridge={ridge}: kkt/bound={worst_kkt:.3f} "
          f"diff={worst_diff:.3e} rss_c={worst_c:.3f} r2/bound={worst_r2:.3f} n_iter_dev_max={int(out['n_iter'].max())} d_iter={d_it}")
    assert worst_kkt <= 2.0, worst_kkt
    assert worst_diff <= EXPRESSION_BOUND[tol], worst_diff
    assert worst_c <= RSS_C_BOUND, worst_c
    assert worst_r2 <= 1.0, worst_r2
    assert d_it <= 1, d_it


@pytest.mark.parametrize("tol", er.GENERIC_TOLS)
@pytest.mark.parametrize("case", er.GENERIC_CASES, ids=[f"K{c[2]}" for c in er.GENERIC_CASES])
def test_generic_solve_meets_the_kkt_bound_and_the_reference(case, tol):
    _check_generic(case, tol)


def test_generic_solve_per_group():
    _check_generic(er.GENERIC_GROUPS_CASE, 1e-10, groups="three")


def test_generic_solve_with_ridge():
    _check_generic(er.RIDGE_CASE[:4], 1e-10, ridge=er.RIDGE_CASE[4])
    # the ridge shrinks: a different answer from the plain solve
    Y, W, _, _, ref = _generic(er.RIDGE_CASE[:4], 1e-10, None, er.RIDGE_CASE[4])
    plain = er.celltype_expression(Y, W, tol=1e-10)
    assert np.abs(plain["expression"] - ref["expression"]).max() > 1e-3 * ref["expression"].max()


def test_one_sweep_reports_no_convergence_where_the_reference_does():
    from flashdeconv_amd.utils.expression import celltype_expression, nnls_gram
    Y, W = er.generic_case(300, 20, 6, 9)
    Y = Y.copy()
    Y[:, 4] = 0.0
    ref = er.celltype_expression(Y, W, max_iter=1)
    out = celltype_expression(Y, W, max_iter=1)
    assert np.array_equal(out["converged"], ref["converged"]) and ref["converged"].sum() == 1 and np.all(out["n_iter"] == 1)
    np.testing.assert_allclose(out["expression"], ref["expression"], rtol=1e-12, atol=0)
    # nnls_gram on the caller's sums: the same solve, with and without q
    A, B, q, _, _ = er.sums(Y, W)
    full = celltype_expression(Y, W)
    got = nnls_gram(A[0], B[0], q=q[0])
    assert set(got) == {"expression", "n_iter", "converged", "rss"} and got["expression"].shape == (6, 20)
    np.testing.assert_allclose(got["expression"], full["expression"], rtol=1e-8, atol=1e-12)
    got3 = nnls_gram(A, B)
    assert set(got3) == {"expression", "n_iter", "converged"} and got3["expression"].shape == (1, 6, 20)
    assert np.array_equal(got3["expression"][0], got["expression"])


# ---------------------------------------------------------------- surface
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_model_method_equals_the_direct_call(output):
    import torch
    from scipy import sparse
    from flashdeconv_amd import FlashDeconv
    from flashdeconv_amd.utils.expression import celltype_expression
    g = load_golden("fit_counts_100x500x5_d64.npz")
    Y, X, coords = g["Y"], g["X"], g["coords"]
    m = FlashDeconv(sketch_dim=64, max_iter=30, random_state=0).fit(Y, X, coords, output=output)
    with pytest.raises(ValueError, match="Unknown what"):
        m.get_celltype_expression(Y, what="counts")
    with pytest.raises(ValueError, match="spots of the fit as rows"):
        m.get_celltype_expression(Y[:50])
    with pytest.raises(ValueError, match="spot_scale must be"):
        m.get_celltype_expression(Y, spot_scale=np.ones(7))
    niches = m.get_spatial_niches(3, random_state=0)["labels"]
    niches = niches.cpu().numpy() if hasattr(niches, "cpu") else np.asarray(niches)
    scale = Y.sum(axis=1) / Y.sum(axis=1).mean()
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)     # noqa: E731
    for what, values in (("proportions", m.proportions_), ("abundances", m.beta_)):
        for Yc in (Y, sparse.csr_matrix(Y)):
            for groups in (None, niches):
                got = m.get_celltype_expression(Yc, what=what, groups=groups)
                want = celltype_expression(Yc, values, groups=groups)
                assert set(got) == set(want) == {"expression", "rss", "tss", "r2", "n_iter", "converged", "gram", "n_rows", "estimable"}
                for key in want:
                    assert np.array_equal(host(got[key]), host(want[key]), equal_nan=True), (what, key)
                lead = (3,) if groups is not None else ()
                assert host(got["expression"]).shape == lead + (5, 500) and host(got["r2"]).shape == lead + (500,)
        scaled = m.get_celltype_expression(Y, what=what, spot_scale=scale)
        want = celltype_expression(Y, host(values) * scale[:, None])
        np.testing.assert_allclose(scaled["expression"], want["expression"], rtol=1e-9, atol=1e-12)
    # every gene is regressed, whatever the fit selected; a gene set of another size is fine
    sub = m.get_celltype_expression(Y[:, :123])
    assert sub["expression"].shape == (5, 123)
    dev = m.get_celltype_expression(torch.as_tensor(Y).cuda(), output="torch", groups=niches)
    assert all(v.is_cuda for v in dev.values()) and dev["expression"].shape == (3, 5, 500)
    assert dev["converged"].dtype == torch.bool and dev["n_iter"].dtype == torch.int32 and dev["n_rows"].dtype == torch.int64
    same = m.get_celltype_expression(Y, groups=niches)
    assert np.array_equal(dev["expression"].cpu().numpy(), same["expression"])


def test_deconvolve_writes_the_expression_on_request_only():
    import flashdeconv_amd as fd
    from flashdeconv_amd.io import prepare_data
    case = datagen.anndata_case()
    kw = dict(cell_type_key="celltype", sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20)
    st0, ref0 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st0, ref0, **kw) is None
    st, ref1 = datagen.anndata_objects(case)
    assert fd.tl.deconvolve(st, ref1, celltype_expression=True, **kw) is None
    assert set(st.uns) == set(st0.uns) | {"flashdeconv_expression", "flashdeconv_expression_r2"}
    assert set(st.obsm) == set(st0.obsm) and set(st.obs.columns) == set(st0.obs.columns)
    assert set(st.uns["flashdeconv_params"]) == set(st0.uns["flashdeconv_params"]) | {"celltype_expression"}
    assert st.uns["flashdeconv_params"]["celltype_expression"] is True
    Y, X, coords, names, genes = prepare_data(st, ref1, cell_type_key="celltype")
    m = fd.FlashDeconv(sketch_dim=64, k_neighbors=4, n_hvg=300, n_markers_per_type=20).fit(Y, X, coords)
    want = m.get_celltype_expression(Y, spot_scale=Y.sum(axis=1) / Y.sum(axis=1).mean())
    ex, r2 = st.uns["flashdeconv_expression"], st.uns["flashdeconv_expression_r2"]
    assert list(ex.index) == [str(x) for x in genes] and list(ex.columns) == [str(t) for t in names] and ex.shape == (470, 5)
    assert list(r2.index) == list(ex.index)
    np.testing.assert_array_equal(ex.values, want["expression"].T)
    np.testing.assert_array_equal(r2.values, want["r2"])
    assert np.all(ex.values >= 0) and np.nanmax(r2.values) <= 1.0
