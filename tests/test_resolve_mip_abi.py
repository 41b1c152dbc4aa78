"""pbr_generate_mips and pbr_resolve_materials_mip in the C ABI: exported from the built library and from the
bounds-checked build, bound in _native, NULL arguments rejected. No device."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from physically_based_renderer_amd import _native as N

SYMBOLS = ("pbr_generate_mips", "pbr_resolve_materials_mip")


def test_symbols_are_declared_exported_and_bound():
    declared = N.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbr_\w+)$", out, flags=re.M))
    lib = N.lib()
    for name in SYMBOLS:
        assert name in declared and name in exported and name in N.SIGNATURES
        assert getattr(lib, name).restype is ctypes.c_int
    assert N.SIGNATURES["pbr_generate_mips"][1] == [ctypes.c_void_p, ctypes.c_void_p]
    assert N.SIGNATURES["pbr_resolve_materials_mip"][1] == [ctypes.c_void_p, ctypes.POINTER(N.AttributesSoA),
                                                           ctypes.POINTER(N.GBufferTargets), ctypes.c_float,
                                                           ctypes.c_void_p]
    assert lib.pbr_abi_version() == 9  # additive: detected by symbol


def test_null_arguments_are_rejected_without_a_device():
    lib = N.lib()
    inv = N.PBR_ERR_INVALID_ARGUMENT
    assert lib.pbr_generate_mips(None, None) == inv
    assert lib.pbr_resolve_materials_mip(None, None, None, 0.0, None) == inv
    a, t = N.AttributesSoA(), N.GBufferTargets()
    assert lib.pbr_resolve_materials_mip(None, ctypes.byref(a), ctypes.byref(t), 0.0, None) == inv


def test_bounds_checked_build_exports_them():
    dbg = os.path.join(os.path.dirname(N.LIB_PATH), "debug_bounds", "libpbrshade.so")
    if not os.path.exists(dbg):
        pytest.skip("bounds-checked build not built (make -C physically_based_renderer_amd/csrc debug-bounds)")
    code = ("from physically_based_renderer_amd import _native as N; L = N.lib(); "
            f"assert all(hasattr(L, s) for s in {SYMBOLS!r}); "
            "assert L.pbr_generate_mips(None, None) == -1; "
            "assert L.pbr_resolve_materials_mip(None, None, None, 0.0, None) == -1; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "PBR_LIB_PATH": dbg}, capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
