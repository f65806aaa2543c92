"""The C ABI with numpy in / numpy out, on both backends (shared by the kernel-level test files; plain helpers, no pytest hooks):

* ``emu``  -- fixture: the host emulation of the unmodified kernel sources (CPU suite) or libtsii_hip.so on the chip (``-m gpu``);
  ``chip``: the chip only;
* ``P(a)`` -- a numpy array as a pointer argument.  On the chip it is staged through device memory around the call;
* ``WS(nbytes)`` -- a workspace of exactly ``nbytes`` with a canary tail;
* ``G(a_or_shape, off=0)`` -- an operand with guard regions in FRONT of and BEHIND it, living at ``16-byte boundary + 4 * off`` bytes
  on either backend (``off=1``: the deliberately misaligned operand that sends a kernel down its ``aligned16`` fall-back).  On the
  chip the whole parent buffer, guards included, is uploaded and downloaded, so a write outside the operand is seen there too;
* the autouse fixture ``_check_workspace_tails`` checks every canary after the test.
"""
import ctypes

import numpy as np
import pytest
import torch

from text_segmentation_image_inpainting_amd import _lib


class _Arr:
    """a numpy array handed to the C ABI: on the GPU backend it is uploaded for the call and copied back afterwards.  ``parent`` /
    ``byte_off``: the array is a view into a staged parent buffer and the kernel gets ``device parent + byte_off``."""

    def __init__(self, a, parent=None, byte_off=0):
        self.a = a
        self.parent = parent
        self.byte_off = byte_off


_MODE = {"gpu": False}
_views = {}      # data address of a G() view -> (parent uint8 buffer, byte offset of the view in it)


def P(a):
    if a is None:
        return None
    if not _MODE["gpu"]:
        return ctypes.c_void_p(a.ctypes.data)
    hit = _views.get(a.ctypes.data)
    return _Arr(a, *hit) if hit is not None else _Arr(a)


class _GpuLib:
    """the bound library with numpy in / numpy out: every array argument is staged through device memory around the call"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            staged, conv = [], []
            for x in args:
                if isinstance(x, _Arr):
                    host = x.parent if x.parent is not None else x.a.reshape(-1).view(np.uint8)
                    t = torch.from_numpy(host).cuda()
                    assert t.data_ptr() % 16 == 0
                    staged.append((host, t))
                    conv.append(ctypes.c_void_p(t.data_ptr() + x.byte_off))
                else:
                    conv.append(x)
            if conv and conv[-1] is None and fn.argtypes and fn.argtypes[-1] is ctypes.c_void_p:
                conv[-1] = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = fn(*conv)
            torch.cuda.synchronize()
            for host, t in staged:
                host[:] = t.cpu().numpy()
            return rc
        return call


def _backend(which):
    if which == "gpu":
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a ROCm GPU")
        _MODE["gpu"] = True
        try:
            yield _GpuLib(_lib.lib())
        finally:
            _MODE["gpu"] = False
        return
    from tests.emu import build_emu
    if not build_emu.available():
        pytest.skip("host clang++ not available")
    yield _lib.bind(ctypes.CDLL(build_emu.build()))


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def emu(request):
    """the library under test: the host emulation of the unmodified kernel sources (CPU suite) or libtsii_hip.so on the chip (-m gpu)"""
    yield from _backend(request.param)


@pytest.fixture(params=[pytest.param("gpu", marks=pytest.mark.gpu)])
def chip(request):
    """libtsii_hip.so on the chip only: workload sizes the emulator would take minutes for"""
    yield from _backend(request.param)


_CANARY = np.float32(-12345.678)
_guarded = []        # (float32 buffer, n): buffer[n:] is canary
_guarded_views = []  # (parent uint8 buffer, start byte, end byte): everything outside [start, end) is canary
_GUARD_BYTES = 256
_CANARY_BYTE = np.uint8(0xA5)


def WS(nbytes):
    n = (int(nbytes) + 3) // 4
    buf = np.zeros(n + 64, np.float32)
    buf[n:] = _CANARY
    _guarded.append((buf, n))
    return buf[:max(n, 1)]


def G(a, off=0, dtype=np.float32):
    """an operand between two guard regions at (16-byte boundary + 4 * off bytes); ``a``: an array (copied in) or a shape (zeros)"""
    if isinstance(a, np.ndarray):
        shape, dtype, src = a.shape, a.dtype, np.ascontiguousarray(a)
    else:
        shape, src = ((a,) if np.isscalar(a) else tuple(a)), None
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    raw = np.empty(nbytes + 2 * _GUARD_BYTES + 16 + 64, np.uint8)
    lead = (-raw.ctypes.data) % 64                      # the parent starts on a 64-byte boundary on the host, as it does on the device
    parent = raw[lead:lead + nbytes + 2 * _GUARD_BYTES + 16]
    parent[:] = _CANARY_BYTE
    start = _GUARD_BYTES + 4 * off
    view = parent[start:start + nbytes].view(dtype).reshape(shape)
    view[...] = 0 if src is None else src
    assert view.ctypes.data % 16 == (4 * off) % 16
    _views[view.ctypes.data] = (parent, start)
    _guarded_views.append((parent, start, start + nbytes))
    return view


def check_guards():
    for buf, n in _guarded:
        assert np.all(buf[n:] == _CANARY), f"a kernel wrote past its {4 * n}-byte workspace"
    for parent, s, e in _guarded_views:
        assert np.all(parent[:s] == _CANARY_BYTE), "a kernel wrote in front of an operand"
        assert np.all(parent[e:] == _CANARY_BYTE), "a kernel wrote behind an operand"


@pytest.fixture(autouse=True)
def _check_workspace_tails():
    _guarded.clear()
    _guarded_views.clear()
    _views.clear()
    yield
    try:
        check_guards()
    finally:
        _guarded.clear()
        _guarded_views.clear()
        _views.clear()
