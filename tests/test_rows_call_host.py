"""What the learner calls of balatro_gym_amd/rows.py share, on the CPU (no GPU, no library).  rows._native_call: the one place where they meet the
C ABI.  A stand-in library object records what it is handed; torch's device guard and current stream are stand-ins too, since neither exists without a
device.  rows._row_pitch: the row pitch of a strided tensor under the two conventions of its callers, and which public call has which."""
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


def _strided(shape, stride, dtype=torch.float32):
    return torch.zeros(4096, dtype=dtype).as_strided(shape, stride)


# (shape, strides) -> (ok, pitch) with lone_row_is_width False, then True.  Read off the code `_row_pitch` replaced -- `_head_logits` (False) and
# `_actor_layer` / `_actor_tile_out` (True) of the commit before it -- and confirmed by running those on these tensors.  Width 60 throughout.
_PITCH_TABLE = [
    ((60,), (1,), (True, 60), (True, 60)),                          # one dimension: the width
    ((1, 60), (64, 1), (True, 64), (True, 60)),                     # [1, 60] of [1, 64]: the two conventions part on a lone row
    ((3, 60), (64, 1), (True, 64), (True, 64)),                     # [3, 60] of [3, 64]
    ((2, 1, 60), (60, 60, 1), (True, 60), (True, 60)),              # [2, 1, 60], contiguous
    # KNOWN DEFECT, pinned because this table is about keeping every caller's pitch: for [2, 1, 60] of [2, 1, 64] True reports 60 for rows that are 64 apart
    # ("The head calls have had it too": left to a pull request of its own).  The fix changes the last pair of THIS row to (True, 64); that is no regression.
    ((2, 1, 60), (64, 64, 1), (True, 64), (True, 60)),
    ((2, 3, 60), (192, 64, 1), (True, 64), (True, 64)),             # [2, 3, 60] over pitch 64
    ((2, 3, 60), (256, 64, 1), (False, 64), (False, 64)),           # [2, 3, 60] of [2, 4, 64]: the leading dimension is not dense
    ((3, 60), (120, 2), (False, 120), (False, 120)),                # a last stride of 2
    ((3, 60), (32, 1), (False, 32), (False, 32)),                   # rows that overlap
    ((1, 60), (8, 1), (False, 8), (True, 60)),                      # a lone row with an arbitrary stride: refused by False alone
    ((0, 60), (60, 1), (True, 60), (True, 60)),                     # an empty leading shape
    ((0, 60), (64, 1), (True, 64), (True, 60)),                     # ... of [0, 64]
    ((2, 0, 60), (0, 64, 1), (True, 64), (True, 60)),
]


@pytest.mark.parametrize("shape,stride,plain,lone", _PITCH_TABLE)
def test_row_pitch(shape, stride, plain, lone):
    t = _strided(shape, stride)
    assert rows._row_pitch(t, 60, False) == plain
    assert rows._row_pitch(t, 60, True) == lone


def test_row_pitch_conventions_of_the_calls():
    """Each public call keeps its convention: a lone row whose stride(-2) its convention reads (False) or ignores (True) is refused for that stride or
    passes every shape check and meets the last refusal, the device's."""
    on_device = "must be a device tensor"
    dense = "dense over"
    lone = _strided((1, 60), (8, 1))                                  # False: pitch 8 < 60, refused; True: pitch 60
    # lone_row_is_width False: encode_rows' out, the logits, the int8 mask
    records = torch.zeros((1, 384), dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must have a contiguous last dimension and leading dimensions that are " + dense):
        rows.encode_rows(records, out=_strided((1, 153), (8, 1)))
    with pytest.raises(ValueError, match=on_device):
        rows.encode_rows(records, out=_strided((1, 153), (160, 1)))
    for call in (lambda lg, mk: rows.sample_actions(lg, mk, seed=1, t=0), lambda lg, mk: rows.sample_actions(lg, mk, seed=1, t=0, epsilon=0.5),
                 lambda lg, mk: rows.evaluate_actions(lg, torch.zeros(1, dtype=torch.int32), mk)):
        with pytest.raises(ValueError, match="logits must have a contiguous last dimension and leading dimensions that are " + dense):
            call(lone, None)
        with pytest.raises(ValueError, match="an int8 mask must have .* a row pitch that is a multiple of 4"):
            call(_strided((1, 60), (64, 1)), _strided((1, 60), (62, 1), torch.int8))       # False: pitch 62; True would say 60 and pass
        with pytest.raises(ValueError, match="logits " + on_device):
            call(_strided((1, 60), (64, 1)), _strided((1, 60), (64, 1), torch.int8))
    # lone_row_is_width True: h and logits_out of the actor calls, h of RowPolicy
    h = _strided((1, 32), (36, 1), torch.bfloat16)                    # True: pitch 32; False would say 36, no multiple of 8
    weight = torch.zeros((60, 32))
    with pytest.raises(ValueError, match="h " + on_device):
        rows.actor_sample(h, weight, seed=1, t=0, logits_out=lone)
    with pytest.raises(ValueError, match="h " + on_device):
        rows.actor_evaluate(h, weight, None, torch.zeros(1, dtype=torch.int32), logits_out=lone)
    with pytest.raises(ValueError, match="h must have .* a row pitch that is a multiple of 8"):
        rows.actor_sample(_strided((2, 32), (36, 1), torch.bfloat16), weight, seed=1, t=0)
    from balatro_gym_amd.policy import RowPolicy
    policy = RowPolicy([], [], [], rows.RowActor(32))
    with pytest.raises(ValueError, match="h " + on_device):
        policy.act(h, seed=1, t=0)
    with pytest.raises(ValueError, match="h must have .* a row pitch that is a multiple of 8"):
        policy.act(_strided((2, 32), (36, 1), torch.bfloat16), seed=1, t=0)
