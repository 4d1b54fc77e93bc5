"""Host-side checks of the halo plan and the halo convolution entry points (no GPU): the plan's size formula, the shapes
the convolution refuses, and empty inputs."""
import ctypes

import pytest


def test_plan_shape_and_size_formula():
    from ptv3_hip.lib import lib
    t, cap = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ptv3_halo_plan_shape(ctypes.byref(t), ctypes.byref(cap)) == 0
    T, CAP = t.value, cap.value
    assert T % 64 == 0 and 0 < CAP < 0xFFFF and CAP >= T          # a tile of isolated sites must fit the fast path
    assert lib.ptv3_halo_plan_bytes(0) == 0
    for m in (1, T - 1, T, T + 1, 5 * T + 9, 100000):
        tiles = -(-m // T)
        want = (tiles * 4 + 15) // 16 * 16 + tiles * CAP * 4 + tiles * T * 27 * 2
        assert lib.ptv3_halo_plan_bytes(m) == want, m
        assert want % 16 == 0


def test_empty_inputs_launch_nothing():
    from ptv3_hip.lib import lib
    assert lib.ptv3_halo_plan_build(None, None, 0, None, 0, None) == 0
    assert lib.ptv3_conv_halo(None, None, None, 0, 64, None, None, None, 0, None, None, None, 0, None, None, None, 1,
                              None) == 0


@pytest.mark.parametrize("c", [0, 16, 48, 96, 128])
def test_refused_channel_counts(c):
    from ptv3_hip.lib import lib
    rc = lib.ptv3_conv_halo(None, None, None, 10, c, None, None, None, 0, None, None, None, 0, None, None, None, 1, None)
    assert rc != 0 and b"must be 32 or 64" in lib.ptv3_last_error()
    assert lib.ptv3_conv_halo_policy(100000, c, c, 27, 1) == 0


def test_refused_arguments():
    from ptv3_hip.lib import lib
    call = lambda **kw: lib.ptv3_conv_halo(None, None, None, kw.get("m", 10), 64, None, None, None, 0, None,  # noqa: E731
                                           kw.get("bns"), None, 0, None, None, kw.get("out2"), kw.get("dtype", 1), None)
    assert call(dtype=7) != 0 and b"bad dtype" in lib.ptv3_last_error()
    assert call(m=-1) != 0 and b"out of range" in lib.ptv3_last_error()
    assert call(m=1 << 31) != 0 and b"out of range" in lib.ptv3_last_error()
    one = (ctypes.c_float * 64)()
    assert call(bns=ctypes.cast(one, ctypes.c_void_p)) != 0 and b"come together" in lib.ptv3_last_error()
    assert call(out2=ctypes.cast(one, ctypes.c_void_p)) != 0 and b"out2 without res" in lib.ptv3_last_error()
    assert call() != 0 and b"are required" in lib.ptv3_last_error()                 # m > 0 with null tensors
    assert lib.ptv3_halo_plan_build(None, None, 10, None, 0, None) != 0 and b"neighbour table" in lib.ptv3_last_error()
    assert lib.ptv3_halo_plan_build(None, None, 1 << 31, None, 0, None) != 0 and b"out of range" in lib.ptv3_last_error()


def test_policy_takes_only_the_shapes_the_kernel_runs(monkeypatch):
    from ptv3_hip.lib import lib
    monkeypatch.delenv("PTV3_CONV_HALO", raising=False)
    assert lib.ptv3_conv_halo_policy(100000, 64, 64, 125, 1) == 0        # the 5^3 stem
    assert lib.ptv3_conv_halo_policy(100000, 32, 64, 27, 1) == 0         # cin != cout
    assert lib.ptv3_conv_halo_policy(300, 64, 64, 27, 1) == 0            # a split-K shape
    monkeypatch.setenv("PTV3_CONV_HALO", "0")
    assert lib.ptv3_conv_halo_policy(100000, 64, 64, 27, 1) == 0
    monkeypatch.setenv("PTV3_CONV_HALO", "2")
    assert lib.ptv3_conv_halo_policy(300, 64, 64, 27, 0) == 1 and lib.ptv3_conv_halo_policy(300, 32, 32, 27, 1) == 1
    assert lib.ptv3_conv_halo_policy(300, 128, 128, 27, 1) == 0
