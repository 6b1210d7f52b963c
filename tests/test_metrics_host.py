"""utils.metrics without a GPU: the module imports, the reference's re-exports are there, and bad shapes are refused before
anything touches the device."""
import numpy as np
import pytest


def test_module_imports_with_reference_names():
    from flashdeconv_amd.utils import metrics
    for name in ("compute_rmse", "compute_mae", "compute_correlation", "compute_jsd", "evaluate_deconvolution",
                 "compute_rare_cell_detection"):
        assert callable(getattr(metrics, name))


def test_utils_reexports_rmse_and_correlation():
    import flashdeconv_amd.utils as utils
    from flashdeconv_amd.utils import compute_correlation, compute_rmse
    assert "compute_rmse" in utils.__all__ and "compute_correlation" in utils.__all__
    assert compute_rmse is utils.metrics.compute_rmse and compute_correlation is utils.metrics.compute_correlation


def test_metrics_symbols_are_bound():
    from flashdeconv_amd import _lib
    for name in ("fdx_metrics_moments_dev", "fdx_metrics_spearman_dev", "fdx_metrics_evaluate_dev"):
        assert name in _lib.SIGNATURES


@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Any attempt to reach the device library fails the test: validation must come first."""
    from flashdeconv_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the GPU library was reached before the shapes were checked")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "require_gpu", boom)


@pytest.mark.parametrize("fn", ["compute_rmse", "compute_mae", "compute_correlation", "compute_jsd", "evaluate_deconvolution",
                                "compute_rare_cell_detection"])
def test_shape_errors_before_gpu(fn, no_gpu_calls):
    from flashdeconv_amd.utils import metrics
    f = getattr(metrics, fn)
    with pytest.raises(ValueError, match=r"\(10, 3\).*\(10, 4\)"):
        f(np.zeros((10, 3)), np.zeros((10, 4)))
    with pytest.raises(ValueError, match=r"2-D.*\(10,\)"):
        f(np.zeros(10), np.zeros(10))
    with pytest.raises(ValueError, match="2-D"):
        f(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)))


def test_size_limit_is_a_value_error(no_gpu_calls):
    from flashdeconv_amd.utils import metrics

    class Big:                               # a shape only: nothing of this size is allocated
        shape = (2 ** 26, 32)
        ndim = 2
    with pytest.raises(ValueError, match="2\\*\\*31 - 1"):
        metrics.compute_rmse(Big(), Big())
