"""The yardstick of tests/test_gpu_leverage.py, checked without a GPU (tests/leverage_ref.py):

  * the long-double reference against a 60-digit mpmath evaluation of x_g^T (Xc Xc^T + reg I)^-1 x_g;
  * LAPACK's own error (the oracle's leverage_scores, float64 gesdd) in units over every case of the GPU file: its maximum is
    the constant L of the bound M * L * unit;
  * the float64 model's forecast of which cases the Cholesky-QR route refuses, with a factor of two to spare either way;
  * teeth: float64 numpy restatements of the device algorithms, each broken in one way, are all rejected by that bound.
"""
import numpy as np
import pytest

import fdx_oracle as orc
import leverage_ref as R


def _ratio(got, case, what="unit"):
    e = R.evaluate(case)
    err = np.abs(np.asarray(got, dtype=np.float64) - e["exact"])
    den = e[what] if what == "unit" else what
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0.0, 0.0, err / den)))


def _rejected(got, case):
    e = R.evaluate(case)
    return bool(np.any(np.abs(got - e["exact"]) > R.bound(e["exact"], e["kappa"])))


@pytest.mark.parametrize("K,G,spread", [(5, 40, 1e2), (12, 70, 1e5), (8, 30, 1e7)])
def test_exact_against_mpmath(K, G, spread):
    """Singular-value spreads of 1e2, 1e5 and 1e7 (kappa, which the ridge caps at s_1 / sqrt(reg): 1e2, 9e4 and 1.2e5).
    Measured: 1.4e-17, 1.8e-15 and 6.6e-16 relative."""
    import mpmath as mp
    reg = 1e-6
    X = R.matrix(R.Case(K, G, "spread", spread))
    kap = R.kappa(X, reg)
    got = R.exact(X, reg)
    with mp.workdps(60):
        Xm = mp.matrix(X.tolist())
        for g in range(G):
            mean = mp.fsum(Xm[k, g] for k in range(K)) / K
            for k in range(K):
                Xm[k, g] -= mean
        inv = (Xm * Xm.T + mp.mpf(reg) * mp.eye(K)) ** -1
        raw = [(Xm[:, g].T * inv * Xm[:, g])[0] for g in range(G)]
        tot = mp.fsum(raw) + mp.mpf(reg)
        rel = max(abs(mp.mpf(float(got[g])) + mp.mpf(float(got[g] - np.longdouble(float(got[g])))) - raw[g] / tot) / (raw[g] / tot)
                  for g in range(G))
    print(f"[test_leverage_host] exact vs mpmath {K}x{G} kappa {kap:g}: {float(rel):.2e}")
    assert rel <= 1e-14


def test_lapack_ratio_over_the_gpu_cases():
    """L = the largest |oracle.leverage_scores - exact| / unit over the file's cases.  One case is left out of L and named here:
    X * 1e4 at reg = 1e-6.  The reference's formula keeps the direction that centring annihilates, whose float64 singular value
    is rounding noise s ~ u |X| sqrt(G K) = 2e-9 there; its weight s^2 / (s^2 + reg) = 4e-12 is LAPACK's relative error on that
    case (700 units), by construction and not by rounding of the factorisation - the same reason regularization = 0 is left out
    altogether.  `exact` and the device's Cholesky-QR route drop that direction."""
    worst, where, left_out = 0.0, None, None
    for c in R.ALL_CASES:
        r = _ratio(orc.leverage_scores(R.matrix(c), c.reg), c)
        if c.kind == "scaled" and c.param > 1.0:
            left_out = r
            continue
        if r > worst:
            worst, where = r, c.id
    print(f"[test_leverage_host] LAPACK / unit: max {worst:.3f} at {where}; X * 1e4: {left_out:.1f}; L = {R.L_LAPACK:g}")
    assert R.L_LAPACK / 3.0 <= worst <= R.L_LAPACK, (worst, where)
    assert left_out > 100.0          # (if this ever drops, the case belongs into L)


def test_model_forecasts_the_refusals_with_room():
    for c in R.QR_WIDE + R.COND_REFUSED + [c for c in R.RANK if c.kind == "twins"]:
        _, refused, w = R.model_qr(R.matrix(c), c.reg)
        assert refused and w < 0.5, (c.id, w)
    for c in R.COND_STANDS + R.QR128 + R.QRBIG + [c for c in R.QR64 if c.G >= c.K - 1]:
        _, refused, w = R.model_qr(R.matrix(c), c.reg)
        assert not refused and w > 2.0, (c.id, w)


def test_unbroken_models_pass_the_bound():
    for c in (R.Case(12, 300), R.Case(12, 300, "kappa", 1e4), R.Case(70, 200), R.Case(17, 129), R.Case(12, 300, "scaled", 1e-6)):
        X = R.matrix(c)
        assert not _rejected(R.model_qr(X, c.reg)[0], c), c.id
        assert not _rejected(R.model_jacobi(X, c.reg), c), c.id


def test_bound_rejects_every_mutant():
    plain, hard, small, ragged = R.Case(12, 300), R.Case(12, 300, "kappa", 2e4), R.Case(12, 300, "scaled", 1e-6), R.Case(17, 129)
    assert hard in R.COND and ragged.G % R.STRIPE == 1
    mutants = {
        "one stripe left out of one Gram entry": (R.model_qr(R.matrix(plain), drop_stripe=(2, 7, 3))[0], plain),
        "one stripe left out of one diagonal Gram entry": (R.model_qr(R.matrix(plain), drop_stripe=(4, 10, 10))[0], plain),
        "CholeskyQR once at kappa 2e4": (R.model_qr(R.matrix(hard), passes=1)[0], hard),
        "weights without + reg": (R.model_jacobi(R.matrix(small), weights_reg=False), small),
        "normalised by the sum alone": (R.model_jacobi(R.matrix(small), norm_reg=False), small),
        "last gene of a ragged stripe left raw": (R.model_qr(R.matrix(ragged), ragged_raw=True)[0], ragged),
        "sig2 from the Gram diagonal before the last rotation": (R.model_jacobi(R.matrix(plain), stale_sig2=True), plain),
    }
    for name, (got, case) in mutants.items():
        r = _ratio(got, case)
        print(f"[test_leverage_host] mutant '{name}': {r:.3g} units (limit {R.M_DEVICE * R.L_LAPACK:g})")
        assert _rejected(got, case), name
