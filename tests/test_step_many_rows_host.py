"""CPU tests (no GPU) of bg_step_many_rows: the header declares it, the library exports it, the ctypes binding lists it, and
BalatroVecEnv.step_many refuses bad arguments of the packed-record call before anything reaches the library."""
import ctypes as C
import os
import re
import types

import pytest

from tests.helpers import ROOT


def _fake_env(n=4):
    """A stand-in for BalatroVecEnv's state (tests/test_cabi_and_host.py): no handle and no `_L` behind it, so a missing check shows up
    as an AttributeError instead of the ValueError expected here."""
    import torch
    return types.SimpleNamespace(_obs=None, _rowbuf=None, num_envs=n, device=torch.device("cpu"))


def test_header_declares_and_library_exports_step_many_rows():
    from balatro_gym_amd import _native as nat, build
    hdr = open(os.path.join(ROOT, "include", "balatro_mi355x.h")).read()
    m = re.search(r"\bint\s+bg_step_many_rows\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_step_many_rows"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 8, params
    assert "const int32_t*" in params[2] and "uint8_t*" in params[3] and "uint64_t" in params[4] and "bg_rollout_stats*" in params[6]
    assert "bg_step_many_rows" in nat.EXPORTS
    # the comment block in front of the declaration says what the path does not produce, and which reference lines it stands for
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    assert "truncated" in doc and "info" in doc and "bg_step_many" in doc and "balatro_env_2.py:616-637" in doc
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert hasattr(L, "bg_step_many_rows"), "libbalatro_mi355x.so does not export bg_step_many_rows"


def test_step_many_rows_wrapper_refuses_bad_arguments():
    """step_many with a RowBuffers: reward / terminated tensors (the records carry them), fewer rows than steps (unless one row: the last
    step's record), and actions that are not [K, N]."""
    import torch
    from balatro_gym_amd.vec_env import BalatroVecEnv, RowBuffers
    n, K = 4, 3
    cpu = torch.device("cpu")
    acts = torch.zeros((K, n), dtype=torch.int32)
    full = RowBuffers(n, cpu, steps=K, row_stride=384)
    for name, dt in (("reward", torch.float64), ("terminated", torch.uint8)):
        with pytest.raises(ValueError, match="packed records already carry"):
            BalatroVecEnv.step_many(_fake_env(n), acts, obs_buffers=full, **{name: torch.zeros((K, n), dtype=dt)})
    with pytest.raises(ValueError, match="fewer rows than steps"):
        BalatroVecEnv.step_many(_fake_env(n), acts, obs_buffers=RowBuffers(n, cpu, steps=K - 1))
    for bad in (torch.zeros(K * n, dtype=torch.int32), torch.zeros((K, n + 1), dtype=torch.int32), torch.zeros((K, n, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"\[K, 4\]"):
            BalatroVecEnv.step_many(_fake_env(n), bad, obs_buffers=full)
    with pytest.raises(ValueError, match="K >= 1"):
        BalatroVecEnv.step_many(_fake_env(n), torch.zeros((0, n), dtype=torch.int32), obs_buffers=full)
    with pytest.raises(ValueError, match="records of 4 envs"):
        BalatroVecEnv.step_many(_fake_env(n), acts, obs_buffers=RowBuffers(n + 1, cpu, steps=K))
    # one row passes the argument checks whatever K (the fake env has no library behind it: the call itself is what fails)
    with pytest.raises(AttributeError):
        BalatroVecEnv.step_many(_fake_env(n), acts, obs_buffers=RowBuffers(n, cpu, steps=1))
    # a namespace that only states `steps` is still the per-key path (tests/test_cabi_and_host.py): its checks, not the records'
    with pytest.raises(ValueError, match="fewer rows than steps"):
        BalatroVecEnv.step_many(_fake_env(n), acts, obs_buffers=types.SimpleNamespace(steps=K - 1))


def test_sharded_step_many_forwards_to_the_local_env():
    from balatro_gym_amd.sharded import ShardedBalatroVecEnv
    calls = []
    local = types.SimpleNamespace(step_many=lambda a, **kw: calls.append((a, kw)) or "out")
    sh = ShardedBalatroVecEnv(8, list(range(8)), rank=1, world=2, local_env_factory=lambda n, seeds, **kw: local)
    assert sh.step_many("acts", obs_buffers="rb") == "out" and calls == [("acts", {"obs_buffers": "rb"})]
