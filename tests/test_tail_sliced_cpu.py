"""Host-side checks of the hidden-sliced block tail (no GPU): the policy with its two environment switches, the
workspace formula, the shapes the entry point refuses and empty inputs."""
import pytest

BF16, F32 = 1, 0


def _call(lib, m=10, c=256, hidden=None, dtype=BF16, groups=8, ws=None, ws_bytes=0):
    return lib.ptv3_block_tail_sliced(None, None, None, None, None, None, None, None, None, None, None, m, c,
                                      4 * c if hidden is None else hidden, 1e-5, dtype, groups, ws, ws_bytes, None)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("PTV3_TAIL_SLICED", "PTV3_TAIL_SLICED_GROUPS", "PTV3_WIDE_ROWS_256"):
        monkeypatch.delenv(k, raising=False)


def test_empty_input_launches_nothing():
    from ptv3_hip.lib import lib
    assert _call(lib, m=0) == 0
    assert _call(lib, m=0, groups=0) == 0


def test_refused_shapes():
    from ptv3_hip.lib import lib
    assert _call(lib, dtype=F32) != 0 and b"bf16 only" in lib.ptv3_last_error()
    assert _call(lib, dtype=7) != 0 and b"bf16 only" in lib.ptv3_last_error()
    for c in (0, 64, 96, 512):
        assert _call(lib, c=c) != 0 and b"not served" in lib.ptv3_last_error()
    assert _call(lib, hidden=512) != 0 and b"not served" in lib.ptv3_last_error()
    assert _call(lib, m=-1) != 0 and b"out of range" in lib.ptv3_last_error()
    assert _call(lib, m=1 << 31) != 0 and b"out of range" in lib.ptv3_last_error()
    for groups in (-1, 3, 5, 6, 32):
        assert _call(lib, groups=groups) != 0 and b"must divide" in lib.ptv3_last_error()
    assert _call(lib, c=128, groups=16) != 0 and b"must divide" in lib.ptv3_last_error()   # hidden / 64 = 8 slices
    assert _call(lib, groups=0) != 0 and b"name the groups" in lib.ptv3_last_error()     # 10 rows: outside the policy
    assert _call(lib) != 0 and b"every tensor is required" in lib.ptv3_last_error()       # m > 0 with null tensors


@pytest.mark.parametrize("groups", [1, 2, 4, 8, 16])
def test_workspace_formula(groups):
    from ptv3_hip.lib import lib
    for m in (0, 1, 245, 1388, 24575):
        want = groups * m * 256 * 4 if groups > 1 else 0
        assert lib.ptv3_block_tail_sliced_workspace_bytes(m, 256, groups) == want


def test_policy_and_its_switches(monkeypatch):
    from ptv3_hip.lib import lib
    policy = lib.ptv3_block_tail_sliced_policy
    assert policy(256, 1024, BF16, 1388) == 8                   # 22 row tiles x 8 groups = 176 workgroups
    assert lib.ptv3_block_tail_sliced_workspace_bytes(1388, 256, 0) == 8 * 1388 * 256 * 4
    assert [policy(256, 1024, BF16, m) for m in (245, 512, 2048, 2049, 2800, 4096)] == [8, 8, 8, 4, 4, 4]
    for m in (245, 512, 1388, 2048, 2049, 2800, 4096):           # one round of the 256 CUs, and no fewer groups than fit
        g = policy(256, 1024, BF16, m)
        assert -(-m // 64) * g <= 256 and (g == 8 or -(-m // 64) * 2 * g > 256), (m, g)
    assert policy(256, 1024, BF16, 244) == 0 and policy(256, 1024, BF16, 4097) == 0    # outside the measured rows
    assert policy(256, 1024, F32, 1388) == 0                    # fp32 stays on the four launches (bitwise tests)
    # C = 128: one group, between the measured row counts at which it is ahead of the cooperative tail
    assert [policy(128, 512, BF16, m) for m in (1388, 5589, 5590, 11000, 16384, 16385)] == [0, 0, 1, 1, 1, 0]
    assert lib.ptv3_block_tail_sliced_workspace_bytes(5590, 128, 0) == 0
    assert policy(128, 512, F32, 5590) == 0 and policy(512, 2048, BF16, 245) == 0
    assert policy(256, 512, BF16, 1388) == 0                    # hidden != 4 c
    assert policy(256, 1024, BF16, 0) == 0
    monkeypatch.setenv("PTV3_TAIL_SLICED_GROUPS", "4")
    assert policy(256, 1024, BF16, 1388) == 4
    monkeypatch.setenv("PTV3_TAIL_SLICED_GROUPS", "3")         # not a divisor of 16: ignored
    assert policy(256, 1024, BF16, 1388) == 8
    monkeypatch.setenv("PTV3_TAIL_SLICED_GROUPS", "16")
    assert policy(256, 1024, BF16, 1388) == 16
    monkeypatch.delenv("PTV3_TAIL_SLICED_GROUPS")
    monkeypatch.setenv("PTV3_TAIL_SLICED", "0")
    assert policy(256, 1024, BF16, 1388) == 0
    monkeypatch.setenv("PTV3_TAIL_SLICED", "2")
    assert policy(256, 1024, BF16, 1) == 8 and policy(256, 1024, BF16, 24575) == 1
    assert policy(256, 1024, BF16, 24576) == 0                  # from there ptv3_block_fusable answers 3
    assert lib.ptv3_block_fusable(256, 1024, BF16, 24576) == 3
    assert policy(256, 1024, F32, 1388) == 0 and policy(64, 256, BF16, 1388) == 0
    assert policy(128, 512, BF16, 1388) == 1 and policy(128, 512, BF16, 24576) == 0
