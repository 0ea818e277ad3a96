"""CPU suite: the AL3D_MATH=auto mode (f16x3 sweeps that re-run out-of-range batches under bf16x6) -- its mode
plumbing, run in fresh child processes, and the argument checks of its flag kernel (no launch, no GPU)."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, math):
    env = dict(os.environ, AL3D_MATH=math, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_auto_mode_imports_as_f16x3_with_recovery_on():
    r = _child("from al3d import detector_ops as D, sweep as S\n"
               "import inspect\n"
               "assert D.MATH == 'f16x3', D.MATH\n"
               "assert D.MATH_AUTO is True\n"
               "assert inspect.signature(S.sweep_embeddings).parameters['recover_range'].default is None\n"
               "print('ok')\n", "auto")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_default_and_explicit_modes_leave_recovery_off():
    for math, want in (("f16x3", "f16x3"), ("bf16x6", "bf16x6")):
        r = _child("from al3d import detector_ops as D\nprint(D.MATH, D.MATH_AUTO)\n", math)
        assert r.returncode == 0 and r.stdout.split() == [want, "False"], (math, r.stdout, r.stderr)


def test_unknown_math_still_fails():
    r = _child("from al3d import detector_ops as D\n", "bogus")
    assert r.returncode != 0
    assert "Al3dError" in r.stderr and "AL3D_MATH='bogus'" in r.stderr


def test_flag_kernel_argument_checks_without_gpu():
    from al3d import lib
    so = lib.load()
    p = ctypes.c_void_p(16)
    f = so.al3d_rows_nonfinite_u8
    assert f(None, 4, 512, 512, p, None) == -1 and b"null pointer" in so.al3d_last_error()
    assert f(p, 4, 512, 512, None, None) == -1 and b"null pointer" in so.al3d_last_error()
    assert f(p, -1, 512, 512, p, None) == -1 and b"bad sizes" in so.al3d_last_error()
    assert f(p, 4, 0, 512, p, None) == -1 and b"bad sizes" in so.al3d_last_error()
    assert f(p, 4, 513, 512, p, None) == -1 and b"bad sizes" in so.al3d_last_error()
    assert f(None, 0, 512, 512, None, None) == 0          # nothing to check: no launch, no pointer needed
    import pytest
    with pytest.raises(lib.Al3dError, match="al3d_rows_nonfinite_u8"):
        lib.call("al3d_rows_nonfinite_u8", None, 2, 7, 9, None, None)
