"""Reads include/mas_hip.h: the ctypes signature of every ``mas_*`` prototype and every integer ``MAS_*`` constant.

The grammar is the header's own habit and nothing beyond it: comments and preprocessor lines aside, a ``typedef struct { } Name;``,
an ``enum { MAS_X = <integer>, ... };`` or one prototype per ``;`` -- ``<type> mas_name(<type> name, ...)`` or ``(void)`` -- with the
types of ``_SCALARS``, ``const char*`` and pointers to anything (two levels at most).  Whatever else it meets (another scalar type, a
function pointer, an unnamed parameter, an enumerator without a value) raises with the declaration's text: a guessed ``argtypes``
entry would load, run, and hand a kernel a truncated stride or a shifted pointer.
"""
import ctypes as C
import functools
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "mas_hip.h")

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "size_t": C.c_size_t,
            "int32_t": C.c_int32, "int64_t": C.c_int64}
_PROTO = re.compile(r"([\w\s*]+?)\b(mas_\w+)\s*\(([^()]*)\)")
_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"
# /* */ without a lazy `.*?` (the header is mostly comment: five times faster) or //
_COMMENT = re.compile(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*")


def _ctype(ctype, structs):
    """the ctypes type of a C type as written (no parameter name), None when this grammar does not cover it; ``structs``: {C name:
    mirror} of the structs the host passes by reference"""
    words = re.findall(r"\w+|\*", ctype)
    cut = words.index("*") if "*" in words else len(words)
    base, stars = " ".join(w for w in words[:cut] if w != "const"), words[cut:].count("*")
    if re.sub(r"[\w\s*]", "", ctype) or not base or not set(words[cut:]) <= {"*", "const"}:
        return None
    if stars == 0:
        return _SCALARS.get(base)
    if stars == 1 and base == "char" and "const" in words[:cut]:
        return C.c_char_p
    if stars == 1:
        return C.POINTER(structs[base]) if base in structs else C.c_void_p
    return C.POINTER(C.c_void_p) if stars == 2 else None


def parse(text, structs):
    """-> (signatures {name: (restype, [argtypes])} in header order, constants {MAS_X: int})"""
    constants, code = {}, []
    for line in _COMMENT.sub(" ", text).splitlines():
        if line.lstrip()[:1] != "#":
            code.append(line)
            continue
        words = line.replace("#", "# ", 1).split()
        if len(words) == 4 and words[1] == "define" and words[2].startswith("MAS_") and re.fullmatch(_INT, words[3]):
            constants[words[2]] = int(words[3], 0)           # a function-like macro's name holds a `(`: never four words that end in an integer

    def enum(m):
        for item in filter(None, (s.strip() for s in m[1].split(","))):
            e = re.fullmatch(rf"(MAS_\w+)\s*=\s*({_INT})", item)
            if not e:
                raise ValueError(f"mas_hip.h: enumerator without an integer value: `{item}`")
            constants[e[1]] = int(e[2], 0)
        return ""
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", "", "\n".join(code))
    text = re.sub(r'extern\s+"C"\s*\{', "", re.sub(r"enum\s*\{([^{}]*)\}\s*;", enum, text))
    *decls, tail = text.split(";")
    if tail.strip() not in ("", "}"):
        raise ValueError(f"mas_hip.h: declaration without `;`: `{tail.strip()}`")

    ctype_of = functools.lru_cache(None)(lambda ctype: _ctype(ctype, structs))     # 1200 parameters, two dozen types

    def bind(text, named):
        ctype, _, name = text.rpartition(" ") if named else (text, "", "_")     # `<type> <name>`: the name is the last word, after a blank
        return ctype_of(ctype) if name.isidentifier() and name != "const" else None
    signatures = {}
    for decl in filter(None, (" ".join(d.split()) for d in decls)):
        m = _PROTO.fullmatch(decl)
        if not m or m[2] in signatures:
            raise ValueError(f"mas_hip.h: not a mas_* prototype the binding can read: `{decl}`")
        params = [] if m[3].strip() == "void" else [a.strip() for a in m[3].split(",")]
        res, args = bind(m[1].strip(), False), [bind(a, True) for a in params]
        if res is None or None in args:
            raise ValueError(f"mas_hip.h: cannot bind `{m[1].strip() if res is None else params[args.index(None)]}` in `{decl}`")
        signatures[m[2]] = (res, args)
    return signatures, constants


def load(structs):
    with open(PATH) as f:
        return parse(f.read(), structs)
