"""Loads lib/libptv3_hip.so and binds it for ctypes from include/ptv3_hip.h itself.

The header is the one declaration of the C ABI: it is parsed once, when this module is imported, into SIGNATURES
(every entry point's restype and argtypes), one ctypes.Structure per `typedef struct` (fields in the header's order)
and one module constant per integer `#define PTV3_*`.  A new entry point is declared in the header and wrapped in
ops.py, nowhere else; tests/test_boundary_cpu.py has a C++ compiler confirm what is derived here."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "ptv3_hip.h")


def library_path():
    return os.environ.get("PTV3_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libptv3_hip.so"))


_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "uint32_t": c_uint32, "size_t": c_size_t,
            "float": c_float, "double": c_double}


def _scalar(name, decl):
    if name not in _SCALARS:
        raise ValueError(f"ptv3_hip.h: unknown type '{name}' in `{decl}`")
    return _SCALARS[name]


def parse_header(text):
    """(functions: name -> (restype, argtypes), structs: name -> Structure class, defines: name -> int).
    Every pointer is a c_void_p, which data_ptr() ints, byref() and ctypes arrays all pass; a `const char*` return is
    a c_char_p.  Strict: a declaration outside this subset of C raises ValueError with its text, none is skipped."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)   # extern "C" { and its }
    defines = {}
    for name, value in re.findall(r"^#define[ \t]+(PTV3_\w+)(.*)$", text, re.M):
        if value.strip():   # the include guard has none
            try:
                defines[name] = int(value, 0)
            except ValueError:
                raise ValueError(f"ptv3_hip.h: `#define {name}{value}` is not an integer") from None
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    structs = {}

    def struct(m):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            base, declarators = re.fullmatch(r"(?:const )?(\w*)(.*)", decl).groups()
            for d in declarators.split(","):
                f = re.fullmatch(r" ?(\*?) ?(\w+)(?:\[(\d+)\])? ?", d)
                if not f:   # bit-field, function pointer, ...
                    raise ValueError(f"ptv3_hip.h: cannot bind field `{decl}` of {m.group(2)}")
                t = c_void_p if f.group(1) else _scalar(base, decl)
                fields.append((f.group(2), t * int(f.group(3)) if f.group(3) else t))
        structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    m = re.search(r"typedef\b.*", text, re.S)
    if m:   # nested or unterminated struct, a typedef of anything else
        raise ValueError(f"ptv3_hip.h: cannot bind `{' '.join(m.group(0).split())[:200]}`")
    *decls, tail = text.split(";")
    if tail.strip():
        raise ValueError(f"ptv3_hip.h: unterminated declaration `{' '.join(tail.split())}`")
    functions = {}
    for decl in filter(None, (" ".join(d.split()) for d in decls)):
        m = re.fullmatch(r"([\w *]+?) ?\b(\w+) ?\(([^()]*)\)", decl)
        if not m:   # function-pointer parameter, two declarations run together, ...
            raise ValueError(f"ptv3_hip.h: cannot bind `{decl}`")
        ret, name, params = m.groups()
        if "*" in ret:
            res = c_char_p if re.fullmatch(r"const char ?\*", ret) else c_void_p
        else:
            res = None if ret == "void" else _scalar(ret, decl)
        args = []
        for p in [] if params.strip() in ("", "void") else params.split(","):
            s = re.fullmatch(r" ?(?:const )?(\w+)(?: \w+)? ?", p)
            if "*" not in p and not s:
                raise ValueError(f"ptv3_hip.h: cannot bind parameter `{p.strip()}` of `{decl}`")
            args.append(c_void_p if "*" in p else _scalar(s.group(1), decl))
        functions[name] = (res, args)
    return functions, structs, defines


try:
    with open(HEADER_PATH) as _f:
        SIGNATURES, STRUCTS, DEFINES = parse_header(_f.read())
except OSError as e:
    raise ImportError(f"ptv3_hip.h not found at {HEADER_PATH}: the ctypes binding is derived from it") from e
globals().update(STRUCTS)   # ptv3_model_desc, ptv3_forward_io, ...
globals().update(DEFINES)   # PTV3_F32, PTV3_BF16, PTV3_ERR_UNSUPPORTED, PTV3_PG_TRUNCATED, ...
BlockTrain, ClsHeadParams, ClsHeadGrads = (STRUCTS[k] for k in ("ptv3_block_train", "ptv3_cls_head_params",
                                                                "ptv3_cls_head_grads"))
ACT_NONE, ACT_GELU, ACT_RELU = (DEFINES[k] for k in ("PTV3_ACT_NONE", "PTV3_ACT_GELU", "PTV3_ACT_RELU"))
ORDER_IDS = {"z": DEFINES["PTV3_ORDER_Z"], "z-trans": DEFINES["PTV3_ORDER_Z_TRANS"],
             "hilbert": DEFINES["PTV3_ORDER_HILBERT"], "hilbert-trans": DEFINES["PTV3_ORDER_HILBERT_TRANS"]}


class _Lib:
    """Lazy handle: importing the package on a box without the .so works, using an op does not."""

    def __init__(self):
        self._dll = None

    def load(self):
        if self._dll is None:
            path = library_path()
            if not os.path.exists(path):
                raise ImportError(
                    f"libptv3_hip.so not found at {path}: build it with `make -C pointcept-keypointdetection_amd` "
                    "(or __graft_entry__.build()); there is no CPU fallback for the PTv3 HIP path")
            dll = ctypes.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = res, args
            self._dll = dll
        return self._dll

    def __getattr__(self, name):
        return getattr(self.load(), name)

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (code {rc}): {self.load().ptv3_last_error().decode()}")


lib = _Lib()
