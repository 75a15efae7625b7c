"""ctypes binding of libmonorec_hip.so, read from include/monorec_hip.h when this module is imported.

The header is the only statement of the C ABI: `ABI`, `DIAGNOSTIC_ABI`, the `ctypes.Structure` classes (`mr_conv_desc` -> `ConvDesc`)
and the integer constants below are built from what `parse_header` reads there, so a new entry point, struct field or constant is an
edit of the header (and of the .hip file behind it), never of this file.  The parser knows exactly the declaration forms the header
uses (its "Conventions" list them) and raises on anything else - a declaration it cannot read is an error, not a hole in the binding.

There is deliberately no fallback: if the HIP library is missing or does not export the whole
ABI, importing the kernels raises - the product path never silently runs on PyTorch/CPU ops.
"""
import ctypes
import os
import re
import types

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "monorec_hip.h")

# the one type table: C scalar -> ctypes.  Every pointer is a c_void_p (it takes ctypes arrays, byref(), None and the integer of
# tensor.data_ptr() alike), but for `const char*` as a return type and a pointer to a struct the header declares WITH a tag
# (`typedef struct mr_x { ... } mr_x;`: a struct the host fills), which is POINTER(its class).  A struct declared without a tag is one
# the device fills (mr_median_stats): it gets a class, to read a copy with, and a pointer to it is a device address like any other
C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
             "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_POINTEES = ("void", "char", "uint8_t", "int16_t", "uint16_t", "uint32_t")      # type names that occur behind a `*` only

_DECLARATIONS = (
    ("enum", re.compile(r"\s*enum\s*\{([^{}]*)\}\s*;")),
    ("struct", re.compile(r"\s*typedef\s+struct\s*(\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;")),
    ("prototype", re.compile(r"\s*([\w\s*]+?)\b(mr_\w+)\s*\(([^(){};]*)\)\s*;")),
)
_DECLARATOR = re.compile(r"(.*?)(\w+)\s*(?:\[([^\]]*)\])?$", re.S)
_EXPRESSION = re.compile(r"(?:\s*(?:0[xX][0-9a-fA-F]+|[0-9]+|MR_[A-Z0-9_]+|[-+()]|\*(?!\*)))+\s*$")      # no `**`: Python's power, no C


def parse_header(text):
    """The C ABI a header text declares: `constants` {name: int} of its `#define`s and enum members, `structs` {C name: ctypes class},
    `abi` / `diagnostic_abi` {entry: (restype, argtypes)} and `abi_c` {entry: (return type, [parameter types])} as C text.  Raises
    ValueError on anything but the forms include/monorec_hip.h lists under "Conventions"."""
    constants, structs, abi, diagnostic_abi, abi_c, host_structs = {}, {}, {}, {}, {}, set()

    def evaluate(expr):
        if not _EXPRESSION.match(expr):
            raise ValueError(f"not an integer expression over literals, + - * ( ) and MR_ names: {expr.strip()!r}")
        try:
            return int(eval(re.sub(r"MR_[A-Z0-9_]+", lambda m: str(constants[m.group()]), expr), {"__builtins__": {}}))
        except (KeyError, SyntaxError, TypeError) as e:
            raise ValueError(f"cannot evaluate {expr.strip()!r}: {e!r}") from e

    def c_type(text):
        """`const float * const*` -> (`const float* const*`, base type name, number of `*`)"""
        words = re.sub(r"\bconst\b", " ", text.replace("*", " ")).split()
        if len(words) != 1 or not (words[0] in C_SCALARS or words[0] in structs or (words[0] in _POINTEES and "*" in text)):
            raise ValueError(f"unknown type {' '.join(text.split())!r}")
        return re.sub(r"\s*\*", "*", " ".join(text.split())), words[0], text.count("*")

    def ctypes_of(text, returned=False):
        spelled, base, stars = c_type(text)
        if stars == 0 and base in C_SCALARS:
            return spelled, C_SCALARS[base]
        if returned:
            if spelled != "const char*":
                raise ValueError(f"unknown return type {spelled!r}")
            return spelled, ctypes.c_char_p
        if stars == 1 and base in host_structs:
            return spelled, ctypes.POINTER(structs[base])
        if stars == 0:
            raise ValueError(f"{spelled!r} by value")
        return spelled, ctypes.c_void_p

    def declare_enum(body):
        for member in body.split(","):
            name, eq, value = member.partition("=")
            if not eq or not re.fullmatch(r"MR_[A-Z0-9_]+", name.strip()):
                raise ValueError(f"enum member {member.strip()!r} is not `MR_NAME = value`")
            constants[name.strip()] = evaluate(value)

    def declare_struct(tag, body, name):
        if tag not in (None, name):
            raise ValueError(f"struct tag {tag!r} of {name}: the tag is the name, or absent for a struct the device fills")
        if tag:
            host_structs.add(name)
        fields = []
        for line in filter(None, (s.strip() for s in body.split(";"))):
            type_text = _DECLARATOR.match(line.split(",")[0]).group(1)      # `int32_t src_h, src_w;`: one type, several declarators
            spelled, ctype = ctypes_of(type_text)
            if "," in line and "*" in spelled:
                raise ValueError(f"several declarators of a pointer type in one line: {line!r}")
            for declarator in line[len(type_text):].split(","):
                m = re.fullmatch(r"\s*(\w+)\s*(?:\[([^\]]*)\])?\s*", declarator)
                if not m:
                    raise ValueError(f"cannot read the field declarator {declarator.strip()!r} of {name}")
                fields.append((m.group(1), ctype if m.group(2) is None else ctype * evaluate(m.group(2))))
        cls = "".join(w.capitalize() for w in name[len("mr_"):].split("_"))
        structs[name] = type(cls, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"`{name}` of include/monorec_hip.h"})

    def declare_prototype(ret, name, params, table):
        ret_c, restype = ctypes_of(ret, returned=True)
        types_c, argtypes = [], []
        if params.strip() != "void":
            for param in params.split(","):
                m = _DECLARATOR.match(param.strip())
                if m.group(3) is not None:
                    raise ValueError(f"array parameter {param.strip()!r} of {name}")
                spelled, ctype = ctypes_of(m.group(1))
                types_c.append(spelled)
                argtypes.append(ctype)
        table[name] = (restype, argtypes)
        abi_c[name] = (ret_c, types_c)

    def declare(pending, table):
        while pending.strip():
            for kind, pattern in _DECLARATIONS:
                m = pattern.match(pending)
                if m:
                    break
            else:
                raise ValueError(f"cannot read the declaration {' '.join(pending.split())[:120]!r}")
            if kind == "enum":
                declare_enum(m.group(1))
            elif kind == "struct":
                declare_struct(m.group(1), m.group(2), m.group(3))
            else:
                declare_prototype(m.group(1), m.group(2), m.group(3), table)
            pending = pending[m.end():]

    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)      # comments go, line numbers stay
    open_ifs, pending = [], ""
    for number, line in enumerate(text.split("\n"), 1):
        try:
            line = line.strip()
            if not line.startswith("#"):
                if "__cplusplus" in open_ifs:
                    if line not in ("", 'extern "C" {', "}"):
                        raise ValueError(f"cannot read {line!r}")
                    continue
                pending += line + "\n"
                if pending.count("{") == pending.count("}") and line.endswith(";"):
                    declare(pending, diagnostic_abi if "MR_DIAGNOSTIC_LIBRARY" in open_ifs else abi)
                    pending = ""
                continue
            if pending.strip():
                raise ValueError(f"cannot read the declaration {' '.join(pending.split())[:120]!r}")
            directive, _, rest = line[1:].strip().partition(" ")
            rest = rest.strip()
            if directive in ("ifdef", "ifndef"):
                # the include guard, `#ifdef __cplusplus`, `#ifdef MR_DIAGNOSTIC_LIBRARY`, and `#ifndef MR_NAME` around a default
                if (directive, rest) not in (("ifndef", "MONOREC_HIP_H"), ("ifdef", "__cplusplus"), ("ifdef", "MR_DIAGNOSTIC_LIBRARY")) \
                        and not (directive == "ifndef" and re.fullmatch(r"MR_[A-Z0-9_]+", rest) and rest not in constants):
                    raise ValueError(f"unknown condition {line!r}")
                open_ifs.append(rest)
            elif directive == "endif" and open_ifs and not rest:
                open_ifs.pop()
            elif directive == "define":
                name, expr = (rest.split(None, 1) + [""])[:2]
                if name == "MONOREC_HIP_H" and not expr:
                    continue
                if not re.fullmatch(r"MR_[A-Z0-9_]+", name) or name in constants:
                    raise ValueError(f"cannot read {line!r}")
                constants[name] = evaluate(expr)
            elif not (directive == "include" and rest in ("<stddef.h>", "<stdint.h>")):
                raise ValueError(f"unknown directive {line!r}")
        except ValueError as e:
            raise ValueError(f"line {number}: {e}") from None
    if pending.strip() or open_ifs:
        raise ValueError(f"unfinished at the end: {' '.join(pending.split())[:120]!r} {open_ifs}")
    return types.SimpleNamespace(constants=constants, structs=structs, abi=abi, diagnostic_abi=diagnostic_abi, abi_c=abi_c)


try:
    with open(HEADER_PATH) as _f:
        HEADER = parse_header(_f.read())
except OSError as _e:
    raise RuntimeError(f"{HEADER_PATH} not found: monorec_amd reads the C ABI of libmonorec_hip.so from this header and does not "
                       "work without it") from _e
except ValueError as _e:
    raise RuntimeError(f"{HEADER_PATH}, {_e}: not a declaration form the binding reads (the header's Conventions list them)") from _e

ABI = HEADER.abi                          # every symbol include/monorec_hip.h declares: (restype, argtypes)
DIAGNOSTIC_ABI = HEADER.diagnostic_abi    # under MR_DIAGNOSTIC_LIBRARY there (python -m monorec_amd.build --timeline): typed when present, never required
ABI_C = HEADER.abi_c                      # both, as the C text of the return and parameter types
globals().update(HEADER.constants)                                        # MR_ABI_VERSION, MR_MAX_SOURCES, ... under their header names
globals().update({c.__name__: c for c in HEADER.structs.values()})        # mr_conv_desc -> ConvDesc, mr_tsdf_ray_view -> TsdfRayView, ...
globals().update({name[len("MR_"):]: value for name, value in HEADER.constants.items()      # the families used without the prefix
                  if name.startswith(("MR_ACT_", "MR_IN_", "MR_TF_", "MR_LAYOUT_", "MR_LAUNCH_", "MR_CV_FAMILY_", "MR_CV_FUSE_"))})
MR_TSDF_TILE = tuple(HEADER.constants["MR_TSDF_TILE_" + a] for a in "XYZ")                    # voxels of one workgroup of mr_tsdf_integrate_f32
MR_TSDF_CLUSTER_TILE = tuple(HEADER.constants["MR_TSDF_CLUSTER_TILE_" + a] for a in "XYZ")    # ... of mr_tsdf_mesh_cluster_vertices_f32
MR_TSDF_MESH_CELLS = (1, 2, 4, 8)    # cluster edges of the mesh entries: the divisors of MR_TSDF_BLOCK (1: the full mesh)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmonorec_hip.so")
_lib = None


def load():
    """Load (once) and type the shared library. Raises RuntimeError if it is missing/incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MR_HIP_LIBRARY") or LIB_PATH      # MR_HIP_LIBRARY: e.g. the timeline-instrumented diagnostic build
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build the gfx950 kernels first (python -m monorec_amd.build or "
            "__graft_entry__.build()). monorec_amd has no CPU/PyTorch fallback for its hot path.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in ABI.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"{path} does not export {name}; rebuild it") from e
        fn.restype = restype
        fn.argtypes = argtypes
    lib.has_diagnostic_forms = True
    for name, (restype, argtypes) in DIAGNOSTIC_ABI.items():
        fn = getattr(lib, name, None)
        if fn is None:
            lib.has_diagnostic_forms = False
            continue
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mr_abi_version() != MR_ABI_VERSION:
        raise RuntimeError("libmonorec_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def check(code, what=""):
    """Turn a non-zero return code into a RuntimeError with hipGetErrorString / MR_ERR text."""
    if code != 0:
        msg = load().mr_error_string(int(code))
        raise RuntimeError(f"{what}: {msg.decode() if msg else code} (code {code})")


def need_cuda(module, t, what):
    """Raise for module `monorec_amd.<module>` unless the tensor `t`, `what` in the message, is on a device."""
    if not t.is_cuda:
        raise RuntimeError(f"monorec_amd.{module}: {what} must be a CUDA (HIP) tensor - there is no CPU fallback")
