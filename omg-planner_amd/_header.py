"""Reader of include/omg_hip.h: the header is the only description of the C ABI and the ctypes bindings are derived from it.

parse(text) -> constants {name: int}, structs {name: ctypes.Structure}, functions {name: (restype, argtypes)}.

Not a C parser.  It knows the four forms the header is written in — `#define NAME <integer expression>`,
`typedef struct omgx_x { scalars, arrays of scalars, pointers } omgx_x;`, prototypes of omgx_* functions, the extern "C" bracket
with the include guard — and raises HeaderError, naming the line, on anything else.  Nothing is skipped: a skipped prototype
would be an entry point that ctypes calls unchecked.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "omg_hip.h"  # as csrc/Makefile finds it: ../../include/omg_hip.h

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
RESTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p}
# The parameter blocks a caller fills on the host and passes by reference: `const <block>* h_x` is POINTER(<block>), so ctypes
# checks what byref() hands over.  Every other pointer (device memory, numpy records, host scalars) is a c_void_p.
PARAM_BLOCKS = ("omgx_chomp_params", "omgx_learner_params", "omgx_plan_iter")
_SKIP = re.compile(r'#\s*(ifn?def\s+\w+|endif|include\s*<\w+\.h>|define\s+\w+)|extern "C" \{|\}')  # guards and the bracket
_EXPR = r"[\w\s()<+*-]+"


class HeaderError(ValueError):
    pass


def _statements(text):
    """(line number, text) of every #define and every declaration up to its `;`, comments and guards removed."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)  # line numbers stay
    stmt, first = "", 0
    for no, line in enumerate(text.split("\n"), 1):
        line = line.strip()
        if stmt or not (line == "" or _SKIP.fullmatch(line)):
            stmt, first = (stmt + " " + line).strip(), first or no
            if line.startswith("#") or (line.endswith(";") and stmt.count("{") == stmt.count("}")):
                yield first, stmt
                stmt, first = "", 0
    if stmt:
        raise HeaderError(f"line {first}: unfinished declaration: {stmt}")


def parse(text: str):
    consts, structs, funcs = {}, {}, {}
    for no, stmt in _statements(text):
        def fail(why):
            return HeaderError(f"line {no}: {why}: {stmt}")

        def value(expr):
            try:
                v = eval(expr, {"__builtins__": {}}, dict(consts))
            except Exception:
                v = None
            if type(v) is not int:
                raise fail(f"`{expr.strip()}` is no integer expression of the #defines before it")
            return v

        def declare(piece, in_struct):
            """`[const] TYPE[*] name` -> [(name, ctype)]; in a struct also `name[N]` and `a, b, c`."""
            m = re.fullmatch(r"\s*(const\s+)?(\w+)\s*(\*?)\s*(\w[\w\s,\[\]()<+*-]*)", piece)
            if not m:
                raise fail(f"cannot read `{piece.strip()}`")
            const, base, star, names = m.groups()
            if base not in SCALARS and not (star and base in ("void", "char", *structs)):
                raise fail(f"unknown type `{base}`")
            ctype = SCALARS[base] if not star else C.c_void_p
            if star and not in_struct and base == "char":
                ctype = C.c_char_p
            if star and not in_struct and const and base in PARAM_BLOCKS and names.startswith("h_"):
                ctype = C.POINTER(structs[base])
            out = []
            for name in names.split(","):
                a = re.fullmatch(rf"\s*(\w+)\s*(?:\[({_EXPR})\])?\s*", name)
                if not a or not in_struct and (a.group(2) or len(out)):
                    raise fail(f"cannot read `{piece.strip()}`")
                out.append((a.group(1), ctype * value(a.group(2)) if a.group(2) else ctype))
            return out

        d = re.fullmatch(rf"#\s*define\s+(\w+)\s+({_EXPR})", stmt)
        s = re.fullmatch(r"typedef struct (\w+) \{(.*)\} \1;", stmt)
        f = re.fullmatch(r"(int|int32_t|int64_t|const char\*) (omgx_\w+)\s*\((.*)\);", stmt)
        if d:
            consts[d.group(1)] = value(d.group(2))
        elif s:
            fields = [fd for piece in s.group(2).split(";") if piece.strip() for fd in declare(piece, True)]
            structs[s.group(1)] = type(s.group(1), (C.Structure,), {"_fields_": fields, "__doc__": f"`{s.group(1)}` of include/omg_hip.h"})
        elif f:
            args = [] if f.group(3).strip() == "void" else [declare(piece, False)[0] for piece in f.group(3).split(",")]
            funcs[f.group(2)] = (RESTYPES[f.group(1)], [ctype for _, ctype in args])
        else:
            raise fail("neither a #define, a struct of scalars, an omgx_* prototype nor the extern \"C\" bracket")
    return consts, structs, funcs
