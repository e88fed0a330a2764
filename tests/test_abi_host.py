"""The ctypes bindings are read from include/amt_hip.h (`_lib.parse_header`): the type mapping on prototypes written out by hand, the
declarations the parser must refuse, the generated structs' layout against the compiler's, and which returns `call` takes for a status."""
import ctypes as C
import os
import re
import subprocess

import pytest

from video2music_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
STRUCTS = {"amt_config": _lib.AmtConfig, "amt_decode_gemm_args": _lib.DecodeGemmArgs, "amt_v2_step_args": _lib.V2StepArgs,
           "amt_v2_decide_args": _lib.V2DecideArgs, "amt_optim_args": _lib.OptimArgs}
P, I, L, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name: (argtypes, restype, status), written by hand from the header's declarations -- not from the parser.  Between them: a char* and
# an int64_t return, a struct pointer and a handle out-pointer, const char* with a host int64_t*, double*, int64_t and float by value,
# a plain-int32_t value return.  Every pointer that names no argument struct is c_void_p: before the bindings were read from the header
# amt_create[1] was POINTER(c_void_p) (and eight more positions POINTER(c_int64) / POINTER(c_double)), so this table fails there.
BY_HAND = {
    "amt_last_error": ([], C.c_char_p, False),
    "amt_decode_step_bytes": ([P, I, I, I], L, False),
    "amt_create": ([C.POINTER(_lib.AmtConfig), P], I, True),
    "amt_load_weight": ([P, C.c_char_p, P, I, P], I, True),
    "amt_generate_profile": ([P, I, P, P, P, P], I, True),
    "amt_add_fwd": ([P, P, P, L, P], I, True),
    "amt_decode_linear_fwd": ([P, P, P, P, P, P, P, P, P, I, I, I, I, F, P], I, True),
    "amt_optim_step": ([C.POINTER(_lib.OptimArgs), P], I, True),
    "amt_optim_plan": ([I], I, False),
}
# the 10 entry points whose int32_t is a value (a count, a route, a plan constant); the header declares every other int32_t return amt_status
INT32_VALUES = {"amt_abi_version", "amt_v2_last_step_launches", "amt_gemm_route", "amt_attn_route", "amt_decode_gemm_ex_lean",
                "amt_moe_wgrad_splits", "amt_rmsnorm_bwd_blocks", "amt_diff_subln_bwd_blocks", "amt_selective_scan_wide_ckpt_steps",
                "amt_optim_plan"}


class _Answers7:
    """Stands in for the loaded library: every entry point returns 7, which `call` must raise on exactly where 7 would be a status."""

    def __getattr__(self, name):
        return (lambda *a: b"seven") if name == "amt_last_error" else (lambda *a: 7)


def _taken_for_a_status(monkeypatch, name):
    monkeypatch.setattr(_lib, "_lib", _Answers7())
    try:
        _lib.call(name)
        return False
    except _lib.AmtError as e:
        assert f"{name} failed (status 7): seven" in str(e)
        return True


@pytest.mark.parametrize("name", sorted(BY_HAND))
def test_type_classes_of_prototypes_written_by_hand(monkeypatch, name):
    argtypes, restype, status = BY_HAND[name]
    assert _lib.SIGNATURES[name] == argtypes
    fn = getattr(_lib.load(), name)                       # what load() put on the function
    assert list(fn.argtypes) == argtypes and fn.restype is restype
    assert _taken_for_a_status(monkeypatch, name) is status


@pytest.mark.parametrize("decl, named", [
    ("int32_t amt_x(size_t n);", "amt_x"),
    ("int32_t amt_x(float v[4]);", "amt_x"),
    ("int32_t amt_x(int32_t);", "amt_x"),
    ("int32_t amt_x(int32_t a, ...);", "amt_x"),
    ("typedef struct amt_x_args { int32_t n; unsigned flags; } amt_x_args;", "amt_x_args"),
])
def test_parser_refuses_what_it_cannot_map(decl, named):
    end = HEADER.rindex("#ifdef __cplusplus")              # inside extern "C", where a declaration would be added
    with pytest.raises(_lib.AmtError, match=named):
        _lib.parse_header(HEADER[:end] + decl + "\n" + HEADER[end:])
    with pytest.raises(_lib.AmtError, match=named):
        _lib.parse_header(HEADER + decl + "\n")


def test_unmodified_header_parses_to_the_modules_tables():
    protos, structs, consts = _lib.parse_header(HEADER)
    def names(table):                                       # a second parse generates struct classes of its own: compare by name
        return {k: [t.__name__ for t in v] for k, v in table.items()}
    assert names({k: v[1] for k, v in protos.items()}) == names(_lib.SIGNATURES) and len(protos) == 114
    assert set(structs) == set(STRUCTS) and consts == _lib.CONST
    assert all(structs[k]._fields_ == STRUCTS[k]._fields_ for k in STRUCTS)
    assert consts["AMT_ABI_VERSION"] == _lib.ABI_VERSION and consts["AMT_GEMM_PRO_GENERIC_FRONT"] == 0x200
    assert not any("(" in k for k in consts) and "AMT_LAYERNORM_BWD_WS_FLOATS" not in consts      # function-like macros are not constants


def test_generated_structs_have_the_compilers_layout(tmp_path):
    lines = []
    for cname, cls in STRUCTS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "amt_hip.h"\nint main() {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # the compiler csrc/build.sh builds the library with; host only
    assert os.path.exists(hipcc), f"{hipcc}: the compiler that built the library is not there"
    subprocess.run([hipcc, "-x", "c++", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    mine = {}
    for cname, cls in STRUCTS.items():
        mine[cname] = C.sizeof(cls)
        mine.update({f"{cname}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    print({k: v for k, v in compiled.items() if "." not in k})
    assert compiled == mine and len(compiled) == 5 + sum(len(cls._fields_) for cls in STRUCTS.values())


def test_call_takes_exactly_the_amt_status_returns_for_statuses(monkeypatch):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    by_type = set(re.findall(r"^(?:int64_t|const char\*) (amt_\w+)\(", text, re.M))
    assert len(by_type) == 18 and not by_type & INT32_VALUES
    values = {name for name in _lib.SIGNATURES if not _taken_for_a_status(monkeypatch, name)}
    assert values == by_type | INT32_VALUES and len(_lib.SIGNATURES) - len(values) == 86
