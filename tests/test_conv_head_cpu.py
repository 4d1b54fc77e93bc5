"""Host-side checks of the fused conv + head entry point (no GPU): the shapes it refuses, empty inputs, and the policy
with its two environment switches."""
import pytest


def _call(lib, m=10, c=64, dtype=1):
    return lib.ptv3_conv_head_halo(None, None, None, m, c, None, None, None, 0, None, None, None, None, None, None, None,
                                   None, None, 1e-5, dtype, None)


def test_empty_input_launches_nothing():
    from ptv3_hip.lib import lib
    assert _call(lib, m=0) == 0


@pytest.mark.parametrize("c", [0, 16, 48, 96, 128])
def test_refused_channel_counts(c, monkeypatch):
    from ptv3_hip.lib import lib
    monkeypatch.setenv("PTV3_CONV_HEAD", "2")
    assert _call(lib, c=c) != 0 and b"must be 32 or 64" in lib.ptv3_last_error()
    assert lib.ptv3_conv_head_halo_policy(100000, c, 1) == 0


def test_refused_arguments():
    from ptv3_hip.lib import lib
    assert _call(lib, dtype=7) != 0 and b"bad dtype" in lib.ptv3_last_error()
    assert _call(lib, m=-1) != 0 and b"out of range" in lib.ptv3_last_error()
    assert _call(lib, m=1 << 31) != 0 and b"out of range" in lib.ptv3_last_error()
    assert _call(lib) != 0 and b"are required" in lib.ptv3_last_error()             # m > 0 with null tensors


def test_policy_and_its_switches(monkeypatch):
    from ptv3_hip.lib import lib
    policy = lib.ptv3_conv_head_halo_policy
    monkeypatch.delenv("PTV3_CONV_HEAD", raising=False)
    monkeypatch.delenv("PTV3_CONV_HEAD_MIN_ROWS", raising=False)
    assert policy(100000, 64, 1) == 1 and policy(21823, 64, 1) == 1
    assert policy(100000, 32, 1) == 0                                  # measured inside the old pair's spread
    assert policy(100000, 64, 0) == 0                                  # fp32 stays on the two kernels
    assert policy(300, 64, 1) == 0                                     # below the row bound
    monkeypatch.setenv("PTV3_CONV_HEAD_MIN_ROWS", "300")
    assert policy(300, 64, 1) == 1 and policy(299, 64, 1) == 0 and policy(300, 64, 0) == 0
    monkeypatch.setenv("PTV3_CONV_HEAD", "0")
    assert policy(100000, 64, 1) == 0
    monkeypatch.setenv("PTV3_CONV_HEAD", "2")
    monkeypatch.delenv("PTV3_CONV_HEAD_MIN_ROWS", raising=False)
    assert policy(1, 64, 0) == 1 and policy(1, 32, 1) == 1 and policy(1, 128, 1) == 0
