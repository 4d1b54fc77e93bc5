"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every declared symbol,
the registry / builder / state_dict surface matches the reference, and the product path refuses to run
without a GPU (no CPU fallback)."""
import ctypes
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "ptv3_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ptv3_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from ptv3_hip.lib import lib, SIGNATURES, library_path
    assert os.path.exists(library_path()), "run __graft_entry__.build() first"
    declared = _declared_symbols()
    assert declared, "header parse failed"
    assert set(declared) == set(SIGNATURES), set(declared) ^ set(SIGNATURES)
    dll = lib.load()
    for name in declared:
        assert getattr(dll, name) is not None
    assert dll.ptv3_version() >= 100


def _host_cxx():
    """A C++ compiler for host code: $CXX, the usual names, else the Makefile's hipcc (a .cpp is host code to it)."""
    makefile = open(os.path.join(ROOT, "pointcept-keypointdetection_amd", "Makefile")).read()
    hipcc = re.search(r"^HIPCC \?= (\S+)", makefile, re.M).group(1)
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", hipcc):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def _type_code(t):
    """Class code of a ctypes type as _ABI_PROBE prints it: v, p, f<bytes>, i<bytes> / u<bytes>."""
    if t is None:
        return "v"
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return "p"
    if t in (ctypes.c_float, ctypes.c_double):
        return f"f{ctypes.sizeof(t)}"
    return f"{'i' if t(-1).value < 0 else 'u'}{ctypes.sizeof(t)}"


_ABI_PROBE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "ptv3_hip.h"
template <class T> void code() {
  typedef typename std::conditional<std::is_void<T>::value, char, T>::type sized;
  if (std::is_void<T>::value) std::printf(" v");
  else if (std::is_pointer<T>::value) std::printf(" p");
  else if (std::is_floating_point<T>::value) std::printf(" f%zu", sizeof(sized));
  else if (std::is_integral<T>::value) std::printf(" %c%zu", std::is_signed<T>::value ? 'i' : 'u', sizeof(sized));
  else std::printf(" ?");
}
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {   // from decltype(&name): no symbol is referenced
  static void print(const char* name) {
    std::printf("%s", name);
    code<R>();
    int each[] = {0, (code<A>(), 0)...};
    (void)each;
    std::printf("\n");
  }
};
#define FN(name) sig<decltype(&name)>::print(#name);
#define STRUCT(name) std::printf(#name " %zu\n", sizeof(name));
#define FIELD(name, f) std::printf(#name "." #f " %zu %zu\n", offsetof(name, f), sizeof(((name*)0)->f));
#define DEFINE(name) std::printf(#name " %lld\n", (long long)(name));
int main() {
"""


def test_compiler_agrees_with_the_derived_binding(tmp_path):
    """What ptv3_hip/lib.py derives from the header's text against what a C++ compiler makes of the same header: the
    class and width of every return and parameter type (pointer / float / signed or unsigned integer / void), sizeof
    every struct, offset and size of every field, the value of every integer define.  The names of functions, structs
    and defines come from regexes of this file, not from the binding, so a declaration the binding lost fails too."""
    import subprocess
    import importlib
    L = importlib.import_module("ptv3_hip.lib")   # the module: ptv3_hip.lib, the attribute, is its handle object
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptv3_hip.h")).read(), flags=re.S)
    functions = _declared_symbols()
    structs = re.findall(r"\}\s*(\w+)\s*;", text)
    defines = re.findall(r"^#define[ \t]+(PTV3_\w+)[ \t]+\S", text, re.M)
    assert set(functions) == set(L.SIGNATURES)
    assert len(structs) == 5 and set(structs) == set(L.STRUCTS)
    assert len(defines) >= 21 and set(defines) == set(L.DEFINES)
    body, want = [], []
    for name in functions:
        res, args = L.SIGNATURES[name]
        body.append(f"FN({name})")
        want.append(" ".join([name, _type_code(res)] + [_type_code(a) for a in args]))
    for name in structs:
        cls = L.STRUCTS[name]
        body.append(f"STRUCT({name})")
        want.append(f"{name} {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            body.append(f"FIELD({name}, {field})")
            want.append(f"{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    for name in defines:
        body.append(f"DEFINE({name})")
        want.append(f"{name} {L.DEFINES[name]}")
    src, exe = tmp_path / "abi_probe.cpp", tmp_path / "abi_probe"
    src.write_text(_ABI_PROBE + "\n".join(body) + "\n}\n")
    r = subprocess.run([cxx, "-std=c++14", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("name,snippet", [
    ("ptv3_a", "int ptv3_ok(int x);\nint ptv3_a(unsigned x, void* stream);"),                    # unknown scalar type
    ("ptv3_b", "int ptv3_b(int (*callback)(int), void* stream);"),                              # function pointer
    ("ptv3_c", "typedef struct { int32_t n; int32_t flags : 3; } ptv3_c;"),                     # bit-field
    ("ptv3_d", "typedef struct { struct { int a; } inner; int b; } ptv3_d;"),                   # nested struct
    ("ptv3_e", "int ptv3_ok(int x);\nint ptv3_e(int x)\n"),                                     # unterminated, at the end
    ("ptv3_f", "int ptv3_f(int x)\nint ptv3_ok(int x);"),                                       # unterminated, inside
    ("PTV3_G", "#define PTV3_G (1 << 4)\nint ptv3_ok(int x);"),                                 # not a plain integer
])
def test_header_parser_refuses_what_it_cannot_bind(name, snippet):
    from ptv3_hip.lib import parse_header
    functions, structs, defines = parse_header("int ptv3_ok(int x);\n#define PTV3_OK 0\n")
    assert list(functions) == ["ptv3_ok"] and not structs and defines == {"PTV3_OK": 0}
    with pytest.raises(ValueError, match=name):
        parse_header(snippet)


def test_derived_structs_construct_positionally_in_header_order():
    """autograd.py and ops.py fill ptv3_block_train and ptv3_cls_head_params positionally: field order is the contract.
    The positions asserted are counted in include/ptv3_hip.h by hand."""
    import importlib
    L = importlib.import_module("ptv3_hip.lib")   # the module: ptv3_hip.lib, the attribute, is its handle object
    assert L.ClsHeadParams is L.ptv3_cls_head_params and L.BlockTrain is L.ptv3_block_train
    assert L.ClsHeadGrads is L.ptv3_cls_head_grads
    p = L.ptv3_cls_head_params(*range(1, 19))
    assert (p.w1, p.bn2_running_mean, p.bn2_eps) == (1, 11, 18.0)
    with pytest.raises(TypeError):
        L.ptv3_cls_head_params(*range(1, 20))
    b = L.ptv3_block_train(*range(1, 81))
    assert (b.n, b.sum_len_sq, b.w_qkv, b.workspace_bytes, b.attn_lse) == (1, 15.0, 25, 79, 80)
    with pytest.raises(TypeError):
        L.ptv3_block_train(*range(1, 82))


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments come back as error codes + message."""
    from ptv3_hip.lib import lib
    rc = lib.ptv3_window_attn_fwd(None, None, None, None, 10, 10, 30, 4, 5, 0.25, None, 0, None)
    assert rc != 0 and b"not divisible" in lib.ptv3_last_error()
    rc = lib.ptv3_gemm(None, None, None, 5, 6, 8, 1, None, None, None, None, None, 0, None, None, None, 0, None, 0,
                       None)
    assert rc != 0 and b"multiple of 4" in lib.ptv3_last_error()
    assert lib.ptv3_gemm_workspace_bytes(100000, 64, 192, 1, 1) == 0      # large M: single pass
    assert lib.ptv3_gemm_workspace_bytes(245, 512, 512, 27, 1) > 0        # deep-stage conv: split over K
    assert lib.ptv3_argsort_workspace_bytes(4, 100000) > 4 * 100000 * 24
    assert lib.ptv3_subm_table_slots(100000) == 262144


def test_no_cpu_fallback():
    from ptv3_hip import ops
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.sfc_encode(torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 3, ["z"])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.gemm(torch.zeros(4, 4), torch.zeros(4, 4))
    from ptv3_hip import autograd as A
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.linear(torch.zeros(4, 8, requires_grad=True), torch.zeros(8, 8), None)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.gemm_tn(torch.zeros(4, 8), torch.zeros(4, 8))


def test_registry_semantics():
    from pointcept.utils.registry import Registry
    R = Registry("things")

    @R.register_module()
    class A:
        def __init__(self, x=1):
            self.x = x

    assert R.get("A") is A and "A" in R and len(R) == 1
    assert R.build(dict(type="A", x=3)).x == 3
    with pytest.raises(KeyError):
        R.register_module(module=A)
    R.register_module(name="A", force=True, module=A)
    R.register_module("alias", module=A)
    assert R.get("alias") is A
    with pytest.raises(KeyError, match="not in the things registry"):
        R.build(dict(type="nope"))
    with pytest.raises(TypeError, match="^A: "):
        R.build(dict(type="A", y=1))
    with pytest.raises(KeyError):
        R.build(dict(x=1))


def test_models_registered_and_state_dict_matches_reference(golden_dir):
    """Keys / shapes / order equal the reference class tree (captured from the reference in
    tests/golden/state_dict_fork_cfg.txt by instantiating its classes in the build container)."""
    from pointcept.models import MODELS, build_model
    from make_golden_cfg import FORK_CFG
    for name in ("PT-v3m1", "OffsetKeypointPTv3", "DefaultSegmentorV2"):
        assert MODELS.get(name) is not None
    cfg = dict(type="OffsetKeypointPTv3", num_keypoints=6, backbone_conf=dict(type="PT-v3m1", **FORK_CFG))
    keep = dict(cfg)
    model = build_model(cfg)
    assert cfg == keep  # build_model deep-copies (builder.py:15-17)
    mine = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_fork_cfg.txt")).read().strip().split("\n")
    assert mine == ref
    assert sum(p.numel() for p in model.backbone.parameters()) == 46158272
    # training and eval both run on the HIP path only: CPU tensors are refused, never silently computed
    import ptv3_scenes as S
    data = S.make_batch([300], in_channels=4, extent=32, seed=0, with_target=6)
    for mode in (True, False):
        with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
            model.train(mode)(data)
    seg = build_model(dict(type="DefaultSegmentorV2", num_classes=19, backbone_out_channels=64,
                           backbone=dict(type="PT-v3m1", **FORK_CFG)))
    assert tuple(seg.seg_head.weight.shape) == (19, 64)


def test_point_dict_surface():
    from pointcept.models.utils.structure import Point
    p = Point(offset=torch.tensor([3, 5]), feat=torch.zeros(5, 2))
    assert p.batch.tolist() == [0, 0, 0, 1, 1] and "batch" in p.keys()
    q = Point(batch=torch.tensor([0, 0, 1]), feat=torch.zeros(3, 2))
    assert q.offset.tolist() == [2, 3]
    q.extra = 5
    assert q["extra"] == 5 and q.pop("extra") == 5
    with pytest.raises(AttributeError):
        q.missing


def test_sync_batchnorm_conversion_is_taken_back():
    """sync_bn=True (engines/train.py:256-257): torch replaces BatchNorm1d by SyncBatchNorm; the package adopts the
    converted modules back around the same tensors (optimizer / DDP / state_dict references stay valid)."""
    import torch
    from pointcept.models.utils.hip_layers import BatchNorm1d, adopt_sync_batchnorm
    seq = torch.nn.Sequential(torch.nn.Linear(4, 8), BatchNorm1d(8, eps=1e-3, momentum=0.01))
    keys = list(seq.state_dict().keys())
    seq = torch.nn.SyncBatchNorm.convert_sync_batchnorm(seq)
    assert isinstance(seq[1], torch.nn.SyncBatchNorm)
    params, bufs = list(seq.parameters()), list(seq.buffers())
    assert adopt_sync_batchnorm(seq) == 1 and adopt_sync_batchnorm(seq) == 0
    assert isinstance(seq[1], BatchNorm1d) and seq[1].sync_group is True
    assert seq[1].eps == 1e-3 and seq[1].momentum == 0.01
    assert all(a is b for a, b in zip(params, seq.parameters())) and all(a is b for a, b in zip(bufs, seq.buffers()))
    assert list(seq.state_dict().keys()) == keys


_GRAFT_PROBE = r"""
import ast, sys, types
cfg_path, pkg = sys.argv[1], sys.argv[2]
sys.path.insert(0, pkg)
import pointcept.utils                      # this package's overlay; its registry module is replaced below


# a registry written apart from the package's, with the interface of the reference's pointcept/utils/registry.py:
# register_module(name=None, force=False, module=None) as a decorator or a call; build(cfg, default_args=None) pops
# cfg["type"] and calls the registered class with the remaining keys
class Registry:

    def __init__(self, name):
        self.name, self.module_dict = name, {}

    def get(self, key):
        return self.module_dict.get(key)

    def register_module(self, name=None, force=False, module=None):
        def register(cls):
            for key in [name] if isinstance(name, str) else (name or [cls.__name__]):
                assert force or key not in self.module_dict, f"{key} is already registered in {self.name}"
                self.module_dict[key] = cls
            return cls
        return register(module) if module is not None else register

    def build(self, cfg, default_args=None):
        args = dict(default_args or {}, **cfg)
        return self.module_dict[args.pop("type")](**args)


registry = types.ModuleType("pointcept.utils.registry")
registry.Registry = Registry
sys.modules[registry.__name__] = registry
pointcept.utils.registry = registry
from pointcept.models import build_model, MODELS
assert type(MODELS) is Registry and MODELS.get("OffsetKeypointPTv3") is not None
model = build_model(ast.literal_eval(open(cfg_path).read()))
print("\n".join(f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()))
"""


def test_models_register_with_a_foreign_registry_and_build_from_the_reference_config():
    """INTEGRATION.md's graft, rehearsed: a Registry class that is not the package's own (a stand-in with the reference's
    registry interface, installed as pointcept.utils.registry before the models are imported) takes this package's
    models, and the model dict of the reference's training config (configs/my_dataset/offset_keypoint_ptv3.py:11-46,
    stored in tests/golden/offset_keypoint_ptv3_model_cfg.txt) builds the offset model with exactly the reference's
    state_dict keys and shapes (tests/golden/state_dict_fork_cfg.txt, listed from the reference's own class)."""
    import subprocess
    import sys
    pkg = os.path.join(ROOT, "pointcept-keypointdetection_amd")
    cfg = os.path.join(ROOT, "tests", "golden", "offset_keypoint_ptv3_model_cfg.txt")
    r = subprocess.run([sys.executable, "-c", _GRAFT_PROBE, cfg, pkg], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [l.strip() for l in r.stdout.strip().splitlines() if l.strip()]
    want = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "state_dict_fork_cfg.txt")) if l.strip()]
    assert got == want


@pytest.mark.parametrize("cfg_name,listing", [("SWIN3D_S3DIS_CFG", "state_dict_swin3d_s3dis.txt"),
                                              ("OFFSET_SWIN3D_CFG", "state_dict_offset_swin3d.txt"),
                                              ("TINY_SWIN3D_GRID_RESSTEM_CFG", "state_dict_swin3d_tiny_grid_resstem.txt")])
def test_swin3d_state_dict_matches_the_reference_classes(cfg_name, listing):
    """Keys, shapes, dtypes and order of "Swin3D-v1m1" / "OffsetKeypointSwin3D" against listings taken from the
    reference's own constructors (tests/golden/make_golden_swin3d.py; its header names the two stem modules whose keys
    come from a MinkowskiEngine stand-in).  The configs restate configs/s3dis/semseg-swin3d-v1m1-0-small.py:11-30 and
    configs/my_dataset/offset_keypoint_swin3d.py:11-40."""
    from ptv3_hip import configs
    from pointcept.models import build_model
    model = build_model(getattr(configs, cfg_name))
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    want = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", listing)) if l.strip()]
    assert got == want


def test_swin3d_constructor_variants_build():
    from ptv3_hip import configs
    from pointcept.models import build_model
    build_model(dict(configs.TINY_SWIN3D_CFG, knn_down=False))            # GridDownsample: built since round 3
    build_model(dict(configs.TINY_SWIN3D_CFG, stem_transformer=False))    # MinkResBlock stem: built since round 3
    from pointcept.models.swin3d import WindowAttention
    # attn_drop: the reference builds nn.Dropout(attn_drop) (swin3d_layers.py:476) and never applies it - accepted, inert
    assert WindowAttention(32, 5, 4, 2, attn_drop=0.1).attn_drop.p == 0.1


def test_offset_models_report_the_reference_training_keys():
    """Every key the reference's offset wrappers put into their training result (InformationWriter logs all of them:
    offset_keypoint_ptv3.py:92-98, offset_keypoint_swin3d.py:92-124) is also produced by this package's classes -
    checked on the source text (the Swin3D class cannot be built here without MinkowskiEngine).  The reference's keys
    were listed from its files by tests/golden/make_golden_boundary.py into tests/golden/reference_train_keys.json."""
    import json
    import re
    reference = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_train_keys.json")))
    pkg = os.path.join(ROOT, "pointcept-keypointdetection_amd", "pointcept", "models")
    for name in ("offset_keypoint_ptv3.py", "offset_keypoint_swin3d.py"):
        want = set(reference[name])
        got = set(re.findall(r'\[f?"(train/[a-z0-9_{}]+)"\]', open(os.path.join(pkg, name)).read()))
        assert want and want <= got, (name, want - got)
