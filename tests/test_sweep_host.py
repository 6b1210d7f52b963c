"""The host reference of one BCD sweep (tests/sweep_ref.py) checked against the oracle, against itself and against planted faults - no
GPU.

What tests/test_gpu_sweep.py relies on: sweep_exact is the oracle's sweep on the integer problems, bit for bit; sweep_longdouble agrees
with it there and with the oracle's first sweep of a real solve; the traversal over planes and padded lists reproduces both in any spot
order; and each fault a sweep kernel can plausibly have - a neighbour slot shifted by one, a halo value of the previous chunk, H of the
next chunk, one b_j left old, the pad row non-zero, the last spot of a ragged tile skipped - trips the comparators on the GPU tests'
own base problem (n = 600, K = 31).  For the rounding comparator the smallest error a fault causes is printed beside the largest E.
"""
import os
import re

import numpy as np
import pytest
from scipy import sparse

import fdx_oracle as orc
import fit_tail_ref as ref
import sweep_ref as sw

N_BASE, K_BASE = 600, 31
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flashdeconv_amd", "csrc")


def _graph(n=N_BASE, seed=11, k=6):
    return sparse.csr_matrix(orc.knn_graph_kdtree(ref.tie_free_coords(n, 2, seed), k))


def _oracle_sweep(A, beta_in, H, XtX, lam, rho):
    A = sparse.csr_matrix(A)
    A.sort_indices()
    b_in = np.ascontiguousarray(beta_in, dtype=np.float64)
    b_out = np.empty_like(b_in)
    diffs, absm = orc.bcd_iteration_c(np.ascontiguousarray(H, dtype=np.float64), np.ascontiguousarray(XtX, dtype=np.float64), b_in, b_out,
                                      np.ascontiguousarray(A.indices.astype(np.int64)), np.ascontiguousarray(A.indptr.astype(np.int64)),
                                      lam, rho)
    return b_out, float(diffs.max() / (absm.max() + 1e-10))


# ------------------------------------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("K", [1, 7, 33])
@pytest.mark.parametrize("coupling,lam,rho", [("none", 1, 0), ("upper", 2, 3)])
def test_exact_sweep_is_the_oracles_sweep(K, coupling, lam, rho):
    A = _graph(300, 3)
    beta, H, XtX = sw.integer_sweep_problem(300, K, 7 + K, coupling)
    info = {}
    got, rc = sw.sweep_exact(A, beta, H, XtX, lam, rho, info)
    want, want_rc = _oracle_sweep(A, beta, H, XtX, float(lam), float(rho))
    sw.assert_sweep_exact(got, want, f"K={K}, {coupling}")
    assert rc == want_rc
    sw.assert_branch_shares(info, rho, f"K={K}, {coupling}")


@pytest.mark.parametrize("K", [1, 7, 33])
def test_longdouble_sweep_is_the_oracles_first_sweep_of_a_solve(K):
    """fdx_oracle.bcd_solve starts from 1 / K and forms XtX, H and rho_eff itself: its first sweep (max_iter = 1) against
    sweep_longdouble from the same start, within 1e-12."""
    n = 300
    A = _graph(n, 3)
    rs = np.random.RandomState(K)
    Xs = rs.rand(K, 12) + 0.1
    Ys = rs.rand(n, K) @ Xs + 0.05 * rs.randn(n, 12)
    want, info = orc.bcd_solve(Ys, Xs, A, lambda_=0.3, rho=0.01, max_iter=1, tol=0.0)
    assert info["n_iterations"] == 1
    XtX, H = Xs @ Xs.T, Xs @ Ys.T
    got, E = sw.sweep_longdouble(A, np.full((n, K), 1.0 / K), H, XtX, 0.3, 0.01 * np.mean(np.diag(XtX)))
    assert np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    sw.assert_sweep_close(want, got, E, f"oracle, K={K}")                # the oracle itself lies within the bound


@pytest.mark.parametrize("K", [1, 7, 33])
def test_longdouble_sweep_agrees_with_the_exact_one(K):
    A = _graph(300, 3)
    beta, H, XtX = sw.integer_sweep_problem(300, K, 7 + K, "upper")
    exact, _ = sw.sweep_exact(A, beta, H, XtX, 2, 3)
    want, E = sw.sweep_longdouble(A, beta, H, XtX, 2, 3)
    assert np.array_equal(np.asarray(want, dtype=np.float64), exact)      # (the quotient rounded once more: same float64 here)
    assert sw.assert_sweep_close(exact, want, E, f"K={K}") <= 1.0


def test_real_problem_meets_its_conditions():
    A = _graph()
    for K in (1, 31, 96, 300):
        beta, H, XtX = sw.real_sweep_problem(N_BASE, K, 77 + K)
        off = np.abs(XtX).sum(1) - np.abs(np.diag(XtX))
        assert (np.diag(XtX) >= 1).all() and (np.diag(XtX) <= 2).all() and (off <= 0.5 * np.diag(XtX)).all() and (beta >= 0).all()
        info = {}
        want, E = sw.sweep_longdouble(A, beta, H, XtX, sw.REAL_LAMBDA, sw.REAL_RHO, info)
        assert min(info["res_above"], info["res_below"], info["res_inside"]) > 0.02, info
        assert E.max() <= 1e-11 * np.abs(want).max(), (K, float(E.max()), float(np.abs(want).max()))


# ------------------------------------------------------------------------------------------------ the traversal and planted faults
def _base(kind, coupling="upper", n=N_BASE, K=K_BASE, A=None):
    A = _graph(n) if A is None else A
    perm = np.random.RandomState(2).permutation(n)
    if kind == "int":
        beta, H, XtX = sw.integer_sweep_problem(n, K, 1000 * K + n, coupling)
        lam, rho, dtype = 2, 3, np.float64
        want, _ = sw.sweep_exact(A, beta, H, XtX, lam, rho)
        E = None
    else:
        beta, H, XtX = sw.real_sweep_problem(n, K, 77 + K)
        lam, rho, dtype = sw.REAL_LAMBDA, sw.REAL_RHO, np.longdouble
        want, E = sw.sweep_longdouble(A, beta, H, XtX, lam, rho)
    lists, deg = ref.padded_lists(A, perm)
    return dict(A=A, perm=perm, beta=beta, H=H, XtX=XtX, lam=lam, rho=rho, dtype=dtype, want=want, E=E, lists=lists, deg=deg, n=n, K=K)


def _walk(c, pad_row=0.0, KC=7, **faults):
    P, Hp = ref.to_planes(c["beta"], c["perm"], pad_row=pad_row), ref.h_to_planes(c["H"], c["perm"])
    out = sw.sweep_planes(P, Hp, c["XtX"], c["lists"], c["deg"], c["n"], c["lam"], c["rho"], KC, dtype=c["dtype"], **faults)
    return np.asarray(sw.from_planes(out, c["perm"], c["n"]), dtype=np.float64)


def _compare(c, got, label):
    if c["E"] is None:
        sw.assert_sweep_exact(got, c["want"], label)
        return 0.0
    return sw.assert_sweep_close(got, c["want"], c["E"], label)


@pytest.mark.parametrize("kind", ["int", "real"])
def test_traversal_over_planes_reproduces_the_reference(kind):
    c = _base(kind)
    assert (c["lists"] == c["n"]).any()                                  # some row is shorter than the width: the pad row is read
    worst = _compare(c, _walk(c), kind)
    assert worst <= 0.05                       # the same arithmetic in longdouble, rounded to float64 once: u / 2 of depth u T / den


def _trips(c, got, label):
    """The comparator fails; for the real problem: the smallest error among the elements the fault moved, beside the largest E."""
    with pytest.raises(AssertionError, match="sweep off" if c["E"] is None else "outside its rounding bound"):
        _compare(c, got, label)
    if c["E"] is not None:
        clean = _walk(c)
        moved = got != clean
        err = np.abs(got.astype(np.longdouble) - c["want"])[moved]
        print(f"{label}: {int(moved.sum())} elements moved, smallest |error| {float(err.min()):.3e}, largest E {float(c['E'].max()):.3e}")
        assert err.min() > c["E"].max()                                  # every element the fault moved is caught on its own


@pytest.mark.parametrize("kind", ["int", "real"])
def test_comparator_fails_on_a_neighbour_slot_shifted_by_one(kind):
    c = _base(kind)
    for p, m in ((0, 0), (255, 2), (c["n"] - 1, 1)):
        _trips(c, _walk(c, slot_shift=(p, m)), f"{kind}: slot {m} of spot {p} shifted")


@pytest.mark.parametrize("kind", ["int", "real"])
def test_comparator_fails_on_a_halo_value_of_the_previous_chunk(kind):
    c = _base(kind)
    got = _walk(c, halo_prev_chunk=True)
    assert (got[:, :7] == _walk(c)[:, :7]).all()                         # the first chunk has no previous one
    _trips(c, got, f"{kind}: halo of type k - KC")


@pytest.mark.parametrize("kind", ["int", "real"])
def test_comparator_fails_on_h_of_the_next_chunk(kind):
    c = _base(kind)
    _trips(c, _walk(c, h_next_chunk=True), f"{kind}: H of type k + KC")


def test_comparator_fails_on_one_b_left_old():
    """Only the real problem can see it: with nothing below the diagonal of XtX the integer problem multiplies every replaced b_j by
    zero - which is what keeps it exact, and why the rounding tier runs at every K of the tiled kernel."""
    c = _base("real")
    _trips(c, _walk(c, stale_b=(K_BASE - 1, 3)), "real: b_3 left old in the last row product")
    _trips(c, _walk(c, stale_b=(8, 7)), "real: b_7 left old in the row product of type 8")
    ci = _base("int")
    _compare(ci, _walk(ci, stale_b=(8, 7)), "int: invisible")


@pytest.mark.parametrize("kind", ["int", "real"])
def test_comparator_fails_on_a_non_zero_pad_row(kind):
    c = _base(kind)
    _trips(c, _walk(c, pad_row=1.0), f"{kind}: pad row 1.0")


@pytest.mark.parametrize("kind", ["int", "real"])
def test_comparator_fails_on_the_last_spot_skipped(kind):
    c = _base(kind)
    got = _walk(c, skip_last=True)
    last = int(c["perm"][c["n"] - 1])
    assert (got[last] == sw.SENTINEL).all() and c["n"] % 256 != 0
    with pytest.raises(AssertionError):
        _compare(c, got, f"{kind}: last spot skipped")


@pytest.mark.parametrize("kind", ["int", "real"])
def test_degree_condition_shows_only_beside_a_non_zero_pad_row(kind):
    """`deg > 0 ? lambda c_k : 0`: a spot without neighbours has c_k = 0 as long as the pad row is zero, so dropping the condition
    alone changes no value on any input - the base problem included - and no test can see it.  What the condition does is keep a spot
    without neighbours independent of the pad row: on a graph with isolated spots and a pad row of 1.0, those spots stay right with
    the condition and go wrong without it."""
    c = _base(kind)
    _compare(c, _walk(c, deg_condition=False), f"{kind}: base problem, condition dropped: the same values")
    rs = np.random.RandomState(4)
    A = _graph(N_BASE).tolil()
    iso = rs.choice(N_BASE, 60, replace=False)
    A[iso, :] = 0
    A[:, iso] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    c = _base(kind, A=A)
    assert (np.diff(c["A"].indptr)[iso] == 0).all()
    _compare(c, _walk(c, deg_condition=False), f"{kind}: isolated spots, condition dropped, pad row zero")
    kept, dropped = _walk(c, pad_row=1.0), _walk(c, pad_row=1.0, deg_condition=False)
    if kind == "int":
        assert np.array_equal(kept[iso], c["want"][iso]) and not np.array_equal(dropped[iso], c["want"][iso])
    else:
        err = lambda g: np.abs(g.astype(np.longdouble) - c["want"])[iso]
        assert (err(kept) <= c["E"][iso]).all() and not (err(dropped) <= c["E"][iso]).all()
    _trips(c, dropped, f"{kind}: isolated spots, condition dropped, pad row 1.0")


def test_rounding_comparator_fails_on_a_nan_and_one_ulp_too_many():
    c = _base("real")
    got = np.asarray(c["want"], dtype=np.float64)
    assert _compare(c, got, "self") <= 1.0
    bad = got.copy()
    i, k = np.unravel_index(np.argmax(c["want"]), got.shape)
    bad[i, k] += 4 * float(c["E"][i, k])
    with pytest.raises(AssertionError, match=f"spot {i}, type {k}"):
        _compare(c, bad, "planted")
    bad = got.copy()
    bad[5, 2] = np.nan
    with pytest.raises(AssertionError, match="spot 5, type 2"):
        _compare(c, bad, "planted NaN")


# ------------------------------------------------------------------------------------------------ the chunk table
def _sweep_chunk():
    """sweep_chunk(K) of csrc/bcd_sweep_inst.cpp, from its chain of `K <= a ? v :`."""
    with open(os.path.join(CSRC, "bcd_sweep_inst.cpp")) as f:
        src = f.read()
    body = src[src.index("constexpr int sweep_chunk(int K)"):]
    body = body[:body.index("\n}\n")]
    expr = re.findall(r"^\s*return\s+(K <[^;]+);", body, re.M)[-1]
    parts = [p.strip() for p in re.split(r"[?:]", expr)]
    assert len(parts) % 2 == 1 and len(parts) >= 5, expr
    rules = []
    for cond, val in zip(parts[0:-1:2], parts[1:-1:2]):
        m = re.fullmatch(r"K (<=|<) (\d+)", cond)
        assert m and re.fullmatch(r"K|\d+", val), (cond, val)
        rules.append((m.group(1), int(m.group(2)), val))
    assert re.fullmatch(r"\d+", parts[-1])

    def chunk(K):
        for op, bound, val in rules:
            if K < bound or (op == "<=" and K == bound):
                return K if val == "K" else int(val)
        return int(parts[-1])
    return chunk


def test_full_k_parametrisation_covers_every_chunk_size():
    import test_gpu_sweep as gpu_file
    chunk = _sweep_chunk()
    assert [chunk(K) for K in (1, 7, 8, 29, 30, 33, 34, 50, 51, 52, 64, 72, 80, 88, 96)] == [1, 7, 8, 8, 7, 7, 6, 2, 2, 8, 8, 6, 4, 4, 2]
    table = {K: chunk(K) for K in sw.FULL_K}
    sizes = sorted(set(table.values()))
    print("sweep_chunk over K = 1..64, 72, 80, 88, 96:", {kc: [K for K in sw.FULL_K if table[K] == kc] for kc in sizes})
    tested = set(gpu_file.K_FULL)
    assert tested == set(sw.FULL_K)
    for kc in sizes:
        ragged = [K for K in sw.FULL_K if table[K] == kc and K % kc != 0]
        whole = [K for K in sw.FULL_K if table[K] == kc and K % kc == 0]
        assert not ragged or tested & set(ragged), f"no tested K with a ragged last chunk of {kc}"
        assert not whole or tested & set(whole), f"no tested K that is a multiple of its chunk {kc}"
    assert all(K in tested for K in gpu_file.K_EDGE) and [table[K] for K in (8, 31, 50, 72)] == [8, 7, 2, 6]
