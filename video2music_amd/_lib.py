"""ctypes binding of ``libamt_hip.so``.  The C ABI is declared once, in ``include/amt_hip.h``: prototypes, argument structs and
constants are read from that file at import (``parse_header``), so a new entry point needs no edit here.

There is deliberately no CPU fallback: if the shared library is missing, or a call returns a
non-zero status, this module raises.  Build the library with ``python -c "import __graft_entry__ as
g; g.build()"`` or ``video2music_amd/csrc/build.sh``.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# AMT_LIB: an alternate build of the same library (tools/ab_build.sh: A/B kernel experiments on one box); default = the in-tree build
LIB_PATH = os.environ.get("AMT_LIB") or os.path.join(_HERE, "lib", "libamt_hip.so")


class AmtError(RuntimeError):
    pass


# ---- the header is the one declaration of the ABI: prototypes, argument structs and constants are read from it ---------------------
_SCALARS = {"int32_t": C.c_int32, "amt_status": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}


def _ctype(ctype, structs, where):
    """ctypes type of a C type of the header.  `structs`: the argument structs a pointer may name ({} inside a struct: every pointer
    field is a c_void_p).  Any other pointer is a c_void_p on purpose: one `const int64_t*` takes a device tensor (`ptr(t)`) in one
    call and a host array (`(c_int64 * n)(...)`, `byref(...)`) in another, and c_void_p accepts all of these."""
    t = re.sub(r"\s*\*\s*", "*", " ".join(ctype.split()))
    if t == "const char*":
        return C.c_char_p
    if t.endswith("*"):
        pointee = t.removeprefix("const ")[:-1]
        return C.POINTER(structs[pointee]) if pointee in structs else C.c_void_p
    if t.removeprefix("const ") not in _SCALARS:
        raise AmtError(f"{where}: no ctypes mapping for the type {t!r} (known: {', '.join(_SCALARS)}, const char*, pointers)")
    return _SCALARS[t.removeprefix("const ")]


def _named(decl, where):
    """(type, name) of a `type name` parameter or field; anything else is refused."""
    found = re.fullmatch(r"(.*[\s*])(\w+)", decl.strip(), re.S)
    if not found or not found.group(1).strip() or re.search(r"[\[(]|\.\.\.", decl):
        raise AmtError(f"{where}: cannot bind {decl.strip()!r} (an array, function pointer, variadic or unnamed declaration?)")
    return found.groups()


def parse_header(text):
    """The ABI `text` (include/amt_hip.h) declares: ({function: (restype, argtypes, returns a status)}, {struct: ctypes.Structure
    class}, {AMT_X: int} for the object-like integer macros).  It reads `type name(args);` and `typedef struct name { ... } name;` and
    raises AmtError, naming the declaration, on anything it cannot map: a binding with a missing type would hand a kernel garbage."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AMT_\w+)[ \t]+(\S+)[ \t]*$", text, re.M):
        try:
            consts[name] = int(value, 0)
        except ValueError:
            pass                                    # not an integer literal: not a constant of the bindings
    text = re.sub(r'^[ \t]*#[^\n]*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
    structs = {}

    def struct(found):
        name, fields = found.group(1), []
        for stmt in filter(None, map(str.strip, found.group(2).split(";"))):
            first, *more = stmt.split(",")          # `int32_t mode, n_tensors;` declares several names
            ctype, field = _named(first, f"struct {name}")
            names = [field] + [m.strip() for m in more]
            if not all(re.fullmatch(r"\w+", n) for n in names):
                raise AmtError(f"struct {name}: cannot bind {stmt!r}")
            fields += [(n, _ctype(ctype, {}, f"struct {name}")) for n in names]
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        return " "
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    protos = {}
    for stmt in map(str.strip, text.split(";")):
        if stmt in ("", "}") or re.fullmatch(r"typedef\s+struct\s+(\w+)\s+\1", stmt):      # "}" closes extern "C"; an opaque handle type
            continue
        alias = re.fullmatch(r"typedef\s+(\w+)\s+(\w+)", stmt)
        found = re.fullmatch(r"(.*?)\b(amt_\w+)\s*\((.*)\)", stmt, re.S)
        if alias:                                   # typedef int32_t amt_status: must agree with _SCALARS
            if alias.group(2) not in _SCALARS or _SCALARS[alias.group(2)] is not _SCALARS.get(alias.group(1)):
                raise AmtError(f"{stmt!r}: a typedef the bindings' type table does not know")
        elif found:
            ret, name, args = found.groups()
            args = [] if args.strip() == "void" else [_ctype(_named(a, name)[0], structs, name) for a in args.split(",")]
            protos[name] = (_ctype(ret, structs, name), args, ret.strip() == "amt_status")
        else:
            raise AmtError(f"cannot read the declaration {' '.join(stmt.split())[:120]!r}")
    unread = set(re.findall(r"\b(amt_\w+)\s*\(", text)) - set(protos)
    if unread:
        raise AmtError(f"declared but not read as prototypes: {sorted(unread)}")
    return protos, structs, consts


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "amt_hip.h")
if not os.path.exists(HEADER_PATH):
    raise AmtError(f"{HEADER_PATH} is missing: the bindings are read from the C header")
with open(HEADER_PATH) as _f:
    _PROTOS, _STRUCTS, CONST = parse_header(_f.read())
SIGNATURES = {name: argtypes for name, (_, argtypes, _) in _PROTOS.items()}       # name -> argtypes
_STATUS = frozenset(name for name, proto in _PROTOS.items() if proto[2])           # declared amt_status: call() raises on non-zero
AmtConfig, DecodeGemmArgs, V2StepArgs, V2DecideArgs, OptimArgs = (
    _STRUCTS[k] for k in ("amt_config", "amt_decode_gemm_args", "amt_v2_step_args", "amt_v2_decide_args", "amt_optim_args"))
ABI_VERSION = CONST["AMT_ABI_VERSION"]              # load() refuses a library that answers another
OPTIM_MAX_TENSORS = CONST["AMT_OPTIM_MAX_TENSORS"]

_lib = None


def load():
    """Returns the loaded CDLL with typed prototypes; raises AmtError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its bundled HIP runtime must be the one in the process before the extension is mapped, or the
    # extension binds to /opt/rocm's copy and the two runtimes do not see each other's device state
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise AmtError(f"{LIB_PATH} is missing: the HIP extension is not built (run __graft_entry__.build()); "
                       "video2music_amd has no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    lib.amt_abi_version.restype = C.c_int32
    have = lib.amt_abi_version()
    if have != ABI_VERSION:
        raise AmtError(f"{LIB_PATH} implements ABI version {have}, these bindings need {ABI_VERSION}: rebuild the library "
                       "(__graft_entry__.build())")
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _PROTOS[name][0]
    _lib = lib
    return lib


def call(name, *args):
    """Calls an entry point and raises AmtError with the library's message on a non-zero status (a return the header declares as
    `amt_status`; any other return is a value and is handed back as it is)."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0 and name in _STATUS:
        msg = lib.amt_last_error()
        raise AmtError(f"{name} failed (status {rc}): {msg.decode() if msg else '?'}")
    return rc


def addr(t):
    """Device address of a (contiguous) tensor as a plain int / None: the form a ctypes Structure field of type c_void_p takes."""
    if t is None:
        return None
    assert t.is_contiguous(), "libamt_hip takes contiguous tensors"
    return t.data_ptr()


def ptr(t):
    """Raw device pointer of a (contiguous) torch tensor, or None."""
    if t is None:
        return None
    assert t.is_contiguous(), "libamt_hip takes contiguous tensors"
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    """The calling thread's current HIP stream as void* (torch.cuda.current_stream().cuda_stream, through the raw accessor: the
    Stream object costs ~7 us per call, which adds up in the host-bound phases -- a few hundred operator calls per generate)."""
    import torch
    try:
        return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    except AttributeError:          # another torch build
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
