"""Argument checks of the ten window-attention entry points of the C ABI (csrc/window_attn.hip, csrc/attn_bwd.hip),
called through ctypes with null or never-dereferenced pointers: every case is answered on the host before any launch,
so no GPU is needed.  One table of cases, applied to every entry that has the argument in question; each case states
the return code, the entry's message prefix and a key word of the message."""
import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
PTR = 4096          # stands for a device pointer whose presence is checked; no case lets a kernel see it

# entry -> (message prefix, argument names in ABI order)
ENTRIES = {
    "fwd": ("window_attn:", "qkv win_order win_inverse out n n_pad c heads patch scale rpe_bias dtype stream"),
    "varlen_fwd": ("window_attn_varlen:", "qkv win_order win_inverse cu num_windows out n n_pad c heads patch scale "
                                          "sum_len_sq dtype stream"),
    "train_fwd": ("window_attn_train:", "qkv win_order win_inverse cu num_windows out lse n n_pad c heads patch scale "
                                        "sum_len_sq dtype stream"),
    "drop_fwd": ("window_attn_drop:", "qkv win_order win_inverse cu num_windows out n n_pad c heads patch scale p_drop "
                                      "seed dtype stream"),
    "rpe_fwd": ("window_attn_rpe:", "qkv win_order win_inverse out n n_pad c heads patch scale grid rpe_table pos_bnd "
                                    "dtype stream"),
    "bwd": ("window_attn_bwd:", "qkv out dout win_order win_inverse dqkv n n_pad c heads patch scale dtype workspace "
                                "workspace_bytes stream"),
    "varlen_bwd": ("window_attn_varlen_bwd:", "qkv out dout win_order win_inverse cu num_windows dqkv n n_pad c heads "
                                              "patch scale dtype workspace workspace_bytes stream"),
    "train_bwd": ("window_attn_train_bwd:", "qkv out dout lse win_order win_inverse cu num_windows dqkv n n_pad c heads "
                                            "patch scale dtype workspace workspace_bytes stream"),
    "drop_bwd": ("window_attn_drop_bwd:", "qkv out dout win_order win_inverse cu num_windows dqkv n n_pad c heads patch "
                                          "scale p_drop seed dtype workspace workspace_bytes stream"),
    "rpe_bwd": ("window_attn_rpe_bwd:", "qkv out dout win_order win_inverse grid rpe_table pos_bnd dqkv dtable n n_pad c "
                                        "heads patch scale dtype workspace workspace_bytes stream"),
}
VARLEN = ("varlen_fwd", "varlen_bwd")
BACKWARD = tuple(e for e in ENTRIES if e.endswith("bwd"))

# a call every entry accepts (one window of 8 slots, head_dim 16); the varlen entries get cu_seqlens, the others none
BASE = dict(qkv=None, win_order=None, win_inverse=None, out=None, dout=None, dqkv=None, workspace=None, stream=None,
            rpe_bias=None, cu=None, num_windows=0, lse=PTR, grid=PTR, rpe_table=PTR, dtable=PTR, pos_bnd=2,
            n=8, n_pad=8, c=32, heads=2, patch=8, scale=0.25, sum_len_sq=0.0, p_drop=0.5, seed=1, dtype=0)

# (case id, argument the entry must have (None: all), overrides, return code, key word); "short" takes one byte off
# the workspace size the library asks for
CASES = [
    ("c_not_divisible", None, dict(c=30, heads=4), ERR_ARG, "not divisible"),
    ("patch_0", None, dict(patch=0), ERR_ARG, "outside [1,16384]"),
    ("patch_16385", None, dict(patch=16385), ERR_ARG, "outside [1,16384]"),
    ("dtype_2", None, dict(dtype=2), ERR_ARG, "bad dtype"),
    ("n_pad_not_a_multiple", "uniform", dict(n_pad=10, patch=4, cu=None), ERR_ARG, "not a multiple"),
    ("cu_missing", "varlen", dict(cu=None), ERR_ARG, "cu_seqlens"),
    ("n_pad_past_windows", "varlen", dict(n_pad=9), ERR_ARG, "cannot be split"),
    ("p_drop_0", "p_drop", dict(p_drop=0.0), ERR_ARG, "p_drop"),
    ("p_drop_1", "p_drop", dict(p_drop=1.0), ERR_ARG, "p_drop"),
    ("lse_missing", "lse", dict(lse=None), ERR_ARG, "lse"),
    ("grid_missing", "grid", dict(grid=None), ERR_ARG, "required"),
    ("table_missing", "rpe_table", dict(rpe_table=None), ERR_ARG, "required"),
    ("dtable_missing", "dtable", dict(dtable=None), ERR_ARG, "required"),
    ("pos_bnd_4097", "rpe_fwd", dict(pos_bnd=4097), ERR_ARG, "pos_bnd"),
    ("table_column_past_lds", "rpe_bwd", dict(pos_bnd=171), ERR_UNSUPPORTED, "exceeds 1024"),
    ("workspace_short", "workspace_bytes", dict(short=1), ERR_ARG, "workspace too small"),
    ("head_dim_8", None, dict(c=16, heads=2, n=8), ERR_UNSUPPORTED, "head_dim 8"),
    ("n_0", "not rpe_bwd", dict(n=0), OK, None),     # the RPE backward zeroes dtable for n = 0: it touches the device
]


def _applies(entry, needs):
    names = ENTRIES[entry][1].split()
    if needs is None:
        return True
    if needs == "uniform":
        return entry not in VARLEN
    if needs == "varlen":
        return entry in VARLEN
    if needs == "not rpe_bwd":
        return entry != "rpe_bwd"
    return needs == entry or needs in names


PARAMS = [pytest.param(entry, over, rc, word, id=f"{entry}-{cid}")
          for entry in ENTRIES for cid, needs, over, rc, word in CASES if _applies(entry, needs)]


def test_the_table_covers_every_entry():
    per_entry = {e: sum(1 for p in PARAMS if p.values[0] == e) for e in ENTRIES}
    assert all(k >= 7 for k in per_entry.values()), per_entry
    assert sum(1 for p in PARAMS if p.values[3] == "head_dim 8") == 10
    assert sum(1 for p in PARAMS if p.values[3] == "workspace too small") == len(BACKWARD) == 5
    assert sum(1 for p in PARAMS if p.values[2] == OK) == 9


@pytest.mark.parametrize("entry,over,rc,word", PARAMS)
def test_entry_point_answers_before_any_launch(entry, over, rc, word):
    from ptv3_hip.lib import lib
    prefix, names = ENTRIES[entry]
    v = dict(BASE)
    if entry in VARLEN:
        v.update(cu=PTR, num_windows=1)
    v.update({k: x for k, x in over.items() if k != "short"})
    if entry == "rpe_bwd":
        need = lib.ptv3_window_attn_rpe_bwd_workspace_bytes(v["n"], v["n_pad"], v["c"], v["heads"], v["patch"],
                                                            v["pos_bnd"], v["dtype"])
    else:
        need = lib.ptv3_window_attn_bwd_workspace_bytes(v["n"], v["n_pad"], v["c"], v["heads"], v["dtype"])
    v["workspace_bytes"] = need - over.get("short", 0)
    got = getattr(lib, "ptv3_window_attn_" + entry)(*[v[k] for k in names.split()])
    assert got == rc, (got, lib.ptv3_last_error())
    if rc == OK:
        return
    msg = lib.ptv3_last_error().decode()
    assert word in msg, msg
    # the head-dim message of the entries that share a body carries the family's name, every other one the entry's own
    assert msg.startswith("window_attn" if word == "head_dim 8" else prefix), msg
