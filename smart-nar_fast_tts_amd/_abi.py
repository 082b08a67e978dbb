"""Reader of ``include/nar_fs2.h``: the header is the one statement of the C ABI, and this turns it into ctypes.

It reads the header's own subset of C, not C: integer ``#define``s, ``typedef struct x x;`` (an opaque handle),
``typedef struct x { fields } x;`` and prototypes.  Anything else — a function pointer, a union, a bit-field, an unknown type
name, an array length it has not seen ``#define``d, a macro or a field defined twice — raises ``HeaderError`` naming the line; nothing is guessed.

The type rule.  Scalars map by spelling: ``int`` c_int, ``int32_t`` c_int32, ``int64_t`` c_int64, ``uint32_t`` c_uint32,
``uint64_t`` c_uint64, ``size_t`` c_size_t, ``float`` c_float, ``double`` c_double.  A ``void`` return is ``None``; ``const char*``
is c_char_p, as return and as parameter.  A pointer to a struct that has a body is ``POINTER(<that Structure>)``.  Every other
pointer is c_void_p: device and host scalar pointers, ``T**``, array parameters (``int32_t out[8]``), opaque handles.  In a
struct every pointer field is c_void_p, a nested struct is that Structure, and arrays keep their lengths (``void* attn[4]`` is
``c_void_p * 4``); an ``NS_*`` constant may be a length.  ``const`` changes nothing.
"""
from __future__ import annotations

import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_POINTEE_ONLY = ("void", "char", "uint8_t")  # known names that only ever stand behind a `*`
_INT = r"(0[xX][0-9a-fA-F]+|[1-9]\d*|0)"
_DEFINE = re.compile(r"(\w+)\s+" + _INT)
_LENGTH = re.compile(_INT)
_WORD = re.compile(r"\w+")
_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)")
_OPAQUE = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)")
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(\w+)\s*\((.*)\)", re.S)
_RETURN = re.compile(r"(\w+)\s*((?:\*\s*)*)")


class HeaderError(ValueError):
    pass


class Abi:
    """``constants`` {macro: int}, ``structs`` {C name: Structure}, ``opaque`` {C name}, ``signatures`` {name: (restype, argtypes)}."""

    def __init__(self, text: str, origin: str = "<header>"):
        self.origin, self.constants, self.structs, self.opaque, self.signatures = origin, {}, {}, set(), {}
        blank = lambda m: " " + "\n" * m.group().count("\n")  # keeps every later line number
        text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)  # one pass: whichever comment opens first owns its text
        lines = re.sub(r"\bconst\b", "     ", text).split("\n")  # `const` changes no type here
        self._text, at, cplusplus = "\n".join(lines), 0, False
        for i, raw in enumerate(lines):
            s = raw.strip()
            if s.startswith("#"):
                word, _, rest = s[1:].strip().partition(" ")
                if s.endswith("\\") or word not in ("define", "ifdef", "ifndef", "endif", "include") or (word == "ifdef" and rest.strip() != "__cplusplus"):
                    self._fail(at, f"preprocessor line outside the subset: {s!r}")
                cplusplus = word == "ifdef" or (cplusplus and word != "endif")
                m = _DEFINE.fullmatch(rest.strip()) if word == "define" else None  # function-like and non-integer macros are skipped
                if m and m[1] in self.constants:
                    self._fail(at, f"{m[1]} is defined twice")
                if m:
                    self.constants[m[1]] = int(m[2], 0)
            if s.startswith("#") or cplusplus:  # `extern "C" {` and its `}`
                lines[i] = " " * len(raw)
            at += len(raw) + 1
        self._text, pos, depth = "\n".join(lines), 0, 0
        for m in re.finditer(r"[{};]", self._text):
            depth += (m.group() == "{") - (m.group() == "}")
            if m.group() == ";" and depth == 0:
                self._statement(self._text[pos:m.start()], pos)
                pos = m.end()
        if self._text[pos:].strip():
            self._fail(pos + len(self._text[pos:]) - len(self._text[pos:].lstrip()), "a declaration without its ';'")

    def _fail(self, pos: int, why: str):
        raise HeaderError(f"{self.origin}:{self._text.count(chr(10), 0, pos) + 1}: {why}")

    def _statement(self, s: str, pos: int):
        pos, s = pos + len(s) - len(s.lstrip()), s.strip()
        m = _OPAQUE.fullmatch(s)
        if m and m[1] == m[2] and m[1] not in self.structs:
            return self.opaque.add(m[1])
        if s.count("{") > 1:
            self._fail(pos + s.index("{", s.index("{") + 1), "a `{` inside braces: only flat struct bodies are read")
        m = _STRUCT.fullmatch(s)
        if m and m[1] == m[3] and m[1] not in self.opaque and m[1] not in self.structs:
            fields, at = [], pos + m.start(2)
            for decl in m[2].split(";"):
                if decl.strip():
                    here = at + len(decl) - len(decl.lstrip())
                    fields += [(name, self._ctype(base, stars, dims, here, "field")) for base, stars, name, dims in self._declarators(decl, here)]
                at += len(decl) + 1
            if len({name for name, _ in fields}) < len(fields):
                self._fail(pos, f"{m[1]} has two fields of one name")
            self.structs[m[1]] = type(m[1].title().replace("_", ""), (C.Structure,), {"_fields_": fields})  # ns_pg_shape -> NsPgShape
            return
        m = _PROTOTYPE.fullmatch(s)
        ret = _RETURN.fullmatch(m[1].strip()) if m else None
        if not ret or m[2] in self.signatures:
            self._fail(pos, f"not a struct typedef, an opaque handle or a (new) prototype: {' '.join(s.split())[:80]!r}")
        args, at = [], pos + m.start(3)
        for param in [] if m[3].strip() == "void" else m[3].split(","):
            here = at + len(param) - len(param.lstrip())
            args += [self._ctype(base, stars, dims, here, "parameter") for base, stars, _, dims in self._declarators(param, here)]
            at += len(param) + 1
        self.signatures[m[2]] = (self._ctype(ret[1], ret[2].count("*"), (), pos, "return"), args)

    def _declarators(self, decl: str, pos: int):
        """``T a, *b, c[4][N]`` -> (T, 0, a, ()), (T, 1, b, ()), (T, 0, c, (4, N)); a parameter is the one-declarator case."""
        decl = decl.strip()
        base = _WORD.match(decl)
        found = [_DECLARATOR.fullmatch(d.strip()) for d in decl[base.end():].split(",")] if base else [None]
        if not all(found):
            self._fail(pos, f"cannot read the declaration {' '.join(decl.split())!r}")
        for d in found:
            dims = _WORD.findall(d[3])
            if not all(_LENGTH.fullmatch(n) or n in self.constants for n in dims):
                self._fail(pos, f"array length of {d[2]!r} is neither an integer nor a macro defined above it")
            yield base[0], d[1].count("*"), d[2], tuple(self.constants[n] if n in self.constants else int(n, 0) for n in dims)

    def _ctype(self, base: str, stars: int, dims: tuple, pos: int, where: str):
        if base not in SCALARS and base not in _POINTEE_ONLY and base not in self.structs and base not in self.opaque:
            self._fail(pos, f"unknown type name {base!r}")
        if where == "field":
            t = C.c_void_p if stars else SCALARS.get(base) or self.structs.get(base)
            for n in reversed(dims):
                t = t and t * n
        elif stars or dims:
            plain = stars == 1 and not dims
            t = C.c_char_p if plain and base == "char" else C.POINTER(self.structs[base]) if plain and base in self.structs else C.c_void_p
        else:
            t = SCALARS.get(base)
            if base == "void" and where == "return":
                return None
        if t is None:
            self._fail(pos, f"{base!r} by value is not allowed in a {where}")
        return t
