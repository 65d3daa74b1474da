"""ctypes harness for the host emulator of the centred-spectrum export / import passes
(tests/emu/emu_spectrum.cpp) -- test infrastructure, built like tests/_emu_mask_grad.py: host clang++, a
plain shared object."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "medical-vision-textural-bias_amd")
SRC = os.path.join(HERE, "emu", "emu_spectrum.cpp")
HDRS = [os.path.join(PKG, "csrc", h) for h in ("fft_core.h", "spectrum.h", "plan_host.h")] + \
       [os.path.join(ROOT, "include", "texbias.h")]
OUT = os.path.join(HERE, "emu", "_build", "libtexbias_emu_spectrum.so")

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = OUT + f".{os.getpid()}.tmp"
        cxx = os.environ.get("TB_EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                               "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                               SRC, "-o", tmp])
        os.replace(tmp, OUT)
    L = C.CDLL(OUT)
    L.tbemu_kspace_export_f32.restype = C.c_int
    L.tbemu_kspace_export_f32.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 3
    L.tbemu_kspace_import_f32.restype = C.c_int
    L.tbemu_kspace_import_f32.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 4
    _lib = L
    return L


def _hwd(spatial):
    from texbias.kprog import geometry
    return geometry(tuple(spatial)).hwd


def kspace_export(x: np.ndarray, n_dims: int, T: int = 8) -> np.ndarray:
    """x: [B, C, *spatial] float32.  Returns K complex64 of x's shape, pre-filled with NaN so an element
    the pass does not write shows."""
    x = np.ascontiguousarray(x, np.float32)
    B, Cc = x.shape[0], x.shape[1]
    spatial = x.shape[2:]
    assert len(spatial) == n_dims
    H, W, D = _hwd(spatial)
    st = np.array([H * W * D, W * D, D], np.int64)
    k = np.full(x.shape, complex(float("nan"), float("nan")), np.complex64)
    rc = lib().tbemu_kspace_export_f32(H, W, D, x.ctypes.data, st.ctypes.data, k.ctypes.data, B, Cc, T)
    if rc:
        raise RuntimeError(f"emulator error {rc}")
    return k


def kspace_import(k: np.ndarray, n_dims: int, pad: int = 0, T: int = 8) -> np.ndarray:
    """k: [B, C, *spatial] complex64.  Returns y float32 [B, C, *spatial[:-1], D + pad], pre-filled with NaN."""
    k = np.ascontiguousarray(k, np.complex64)
    B, Cc = k.shape[0], k.shape[1]
    spatial = k.shape[2:]
    assert len(spatial) == n_dims
    H, W, D = _hwd(spatial)
    ld = D + pad
    st = np.array([H * W * ld, W * ld, ld], np.int64)
    y = np.full(k.shape[:-1] + (ld,), float("nan"), np.float32)
    rc = lib().tbemu_kspace_import_f32(H, W, D, k.ctypes.data, y.ctypes.data, st.ctypes.data, pad, B, Cc, T)
    if rc:
        raise RuntimeError(f"emulator error {rc}")
    return y
