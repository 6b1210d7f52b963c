"""CPU-only tests of the per-spot diagnostics surface: the getter's errors and the ctypes mirrors of the two structs that grew."""
import ctypes
import os

import pytest

from conftest import ROOT


def test_get_spot_residuals_needs_a_fit():
    from flashdeconv_amd import FlashDeconv
    m = FlashDeconv()
    assert m.spot_diagnostics_ is None
    with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
        m.get_spot_residuals()
    with pytest.raises(RuntimeError, match=r"Model has not been fitted\. Call fit\(\) first\."):
        m.get_spot_residuals(relative=False)


def test_fit_structs_mirror_the_header(tmp_path):
    """fdx_fit_params / fdx_fit_info end in spot_diag_out_dev / diag_ms: the ctypes structures must have the C sizes and put the
    two new fields where the compiler does."""
    import shutil
    import subprocess
    from flashdeconv_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fdx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(fdx_fit_params), sizeof(fdx_fit_info), '
                   'offsetof(fdx_fit_params, spot_diag_out_dev), offsetof(fdx_fit_info, diag_ms)); return 0; }\n')
    exe = tmp_path / "t"
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib.FitParams), ctypes.sizeof(_lib.FitInfo), _lib.FitParams.spot_diag_out_dev.offset,
                     _lib.FitInfo.diag_ms.offset]
    assert _lib.FitParams._fields_[-1][0] == "spot_diag_out_dev" and _lib.FitInfo._fields_[-1][0] == "diag_ms"
    assert _lib.FitParams().spot_diag_out_dev is None and _lib.FitInfo().diag_ms == 0.0       # a zeroed struct: the feature is off
    assert _lib.load().fdx_version() >= 201
