"""rows._native_call on the CPU (no GPU, no library): the one place where the learner calls of balatro_gym_amd/rows.py meet the C ABI.  A stand-in
library object records what it is handed; torch's device guard and current stream are stand-ins too, since neither exists without a device."""
import contextlib
import ctypes as C

import pytest
import torch

from balatro_gym_amd import _native as nat, rows

STREAM = 0x5EED0


class _Fn:
    """bg_fake(a, b, kernel_ms_out, stream) -> rc, with its argtypes declared as _native.load() declares every entry point's."""
    argtypes = (C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p)

    def __init__(self, lib):
        self.lib = lib

    def __call__(self, *args):
        self.lib.calls.append(args)
        if args[-2] is not None:   # the float out-parameter: ctypes.byref(c_float)
            args[-2]._obj.value = self.lib.ms
        return self.lib.rc


class _Lib:
    """bg_fake; bg_last_error(NULL) -> the text of the last refusal."""

    def __init__(self, rc=0, ms=1.25):
        self.rc, self.ms, self.calls = rc, ms, []
        self.bg_fake = _Fn(self)

    def bg_last_error(self, handle):
        assert handle is None
        return b"bg_fake: m out of range"


@pytest.fixture
def lib(monkeypatch):
    L, guards, loads = _Lib(), [], []

    @contextlib.contextmanager
    def guard(dev):
        guards.append(dev)
        yield

    class _Stream:
        cuda_stream = STREAM

    monkeypatch.setattr(torch.cuda, "device", guard)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev: _Stream())
    monkeypatch.setattr(nat, "load", lambda: loads.append(1) or L)
    L.guards, L.loads = guards, loads
    return L


def test_native_call(lib):
    # 1. the stream, and with timing a float out-parameter, are handed over behind the caller's arguments; the device guard is the tensors' device
    dev = torch.device("cuda:3")
    assert rows._native_call("bg_fake", dev, (7, 8), "R", False) == "R"
    (a, b, ms, stream), = lib.calls
    assert (a, b) == (7, 8) and ms is None, "without timing kernel_ms_out is NULL"
    assert stream == STREAM, "the last argument is torch's current stream of the device"
    assert lib.guards == [dev], "the call runs with the tensors' device current"
    rows._native_call("bg_fake", dev, (7, 8), "R", True)
    assert isinstance(lib.calls[1][2]._obj, C.c_float), "with timing kernel_ms_out points at a float"
    assert lib.calls[1][3] == STREAM

    # 2. the documented shapes of the timing return
    assert rows._native_call("bg_fake", dev, (1, 2), "R", True) == ("R", 1.25), "a single result: (result, ms)"
    assert rows._native_call("bg_fake", dev, (1, 2), ("A", "B"), True) == ("A", "B", 1.25), "a tuple: the milliseconds are appended"
    assert rows._native_call("bg_fake", dev, (1, 2), ("A", "B"), False) == ("A", "B")
    assert rows._native_call("bg_fake", dev, (1, 2), (), True) == (1.25,) and rows._native_call("bg_fake", dev, (1, 2), (), False) == ()

    # 3. a non-zero return: NativeError with the name of the function called and bg_last_error's text
    lib.rc = -2
    with pytest.raises(nat.NativeError, match=r"^bg_fake failed \(-2\): bg_fake: m out of range$"):
        rows._native_call("bg_fake", dev, (1, 2), "R", False)
    with pytest.raises(nat.NativeError, match=r"bg_fake failed \(-2\)"):
        rows._native_call("bg_fake", dev, (1, 2), ("A",), True)

    lib.bg_fake.argtypes = None   # (addresses travel as ints: a function without declared argtypes is refused before it is called)
    n = len(lib.calls)
    with pytest.raises(nat.NativeError, match="bg_fake has no argtypes"):
        rows._native_call("bg_fake", dev, (1, 2), "R", False)
    assert len(lib.calls) == n
    lib.bg_fake.argtypes = _Fn.argtypes

    # 4. an empty shape: nothing is loaded, called or switched (a call would raise: rc is still -2), the time is 0.0
    del lib.calls[:], lib.guards[:], lib.loads[:]
    assert rows._native_call("bg_fake", dev, (), "R", False, empty=True) == "R"
    assert rows._native_call("bg_fake", dev, (), "R", True, empty=True) == ("R", 0.0)
    assert rows._native_call("bg_fake", dev, (), ("A", "B"), True, empty=True) == ("A", "B", 0.0)
    assert lib.loads == [] and lib.calls == [] and lib.guards == []
