"""Reads the text of include/graphode.h into ctypes: the one statement of the C ABI that _lib.py binds.

parse(text) -> (constants, structs, signatures).  The header is plain C99 in a narrow style (scalars, pointers, arrays,
earlier structs by value); a declaration outside that style raises HeaderError with its text - nothing is ever skipped,
because a declaration bound wrongly hands the kernels garbage.
"""
import ctypes
import keyword
import re

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "float": ctypes.c_float, "double": ctypes.c_double}

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(GODE_\w+)[ \t]+(\d+)[ \t]*$", re.M)
_STRUCT = re.compile(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_MEMBER = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\*\s*)*(?:const\s+)?(\w+)\s*(?:\[\s*(\w+)\s*\])?")
_PROTO = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(gode_\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"(const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)?\s*(\[\s*\])?")


class HeaderError(ValueError):
    pass


def _ctype(base, depth, structs, decl):
    """ctypes type of an object of C type `base` behind `depth` stars: a scalar or an earlier struct, or c_void_p."""
    known = SCALARS.get(base) or structs.get(base)
    if known is None and not (depth and base in ("void", "char")):
        raise HeaderError("graphode.h: unknown type '%s' in: %s" % (base, decl))
    return ctypes.c_void_p if depth else known


def _struct_fields(body, constants, structs, tag):
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        where = "%s { %s; }" % (tag, decl)
        m = _MEMBER.fullmatch(decl)
        base, rest = m.groups() if m else ("", decl)
        for declarator in rest.split(","):
            m = _DECLARATOR.fullmatch(declarator.strip()) if base else None
            if m is None:                                      # a bit-field, a function pointer, `unsigned int`, ...
                raise HeaderError("graphode.h: cannot read member declarator '%s' in: %s" % (declarator.strip(), where))
            star, name, bound = m.groups()
            ctype = _ctype(base, 1 if star else 0, structs, where)
            if bound is not None:
                if not (bound.isdecimal() or bound in constants):
                    raise HeaderError("graphode.h: array bound '%s' is neither decimal nor a constant in: %s" % (bound, where))
                ctype = ctype * (int(bound) if bound.isdecimal() else constants[bound])
            fields.append((name + "_" if keyword.iskeyword(name) else name, ctype))
    return fields


def _signature(decl, structs):
    m = _PROTO.fullmatch(decl)
    if m is None:
        raise HeaderError("graphode.h: cannot read declaration: %s" % decl)
    base, star, name, params = m.groups()
    if base == "void" and not star:
        restype = None
    else:
        restype = ctypes.c_char_p if base == "char" and star else _ctype(base, len(star), structs, decl)
    argtypes = []
    for param in ([] if params.strip() == "void" else params.split(",")):
        m = _PARAM.fullmatch(param.strip())
        if m is None:                                           # a function pointer, `unsigned int`, `struct x`, ...
            raise HeaderError("graphode.h: cannot read parameter '%s' of: %s" % (param.strip(), decl))
        const, base, stars, _, brackets = m.groups()
        depth = stars.count("*") + (1 if brackets else 0)
        if depth == 1 and base == "char" and const:
            argtypes.append(ctypes.c_char_p)
        elif depth == 1 and base in structs:
            argtypes.append(ctypes.POINTER(structs[base]))
        else:
            argtypes.append(_ctype(base, depth, structs, decl))
    return name, (restype, argtypes)


def parse(text):
    """Header text -> ({GODE_NAME: int}, {typedef name: Structure class}, {function: (restype, argtypes)})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {k: int(v) for k, v in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text)
    structs = {}

    def add_struct(m):
        body, tag = m.groups()
        structs[tag] = type(tag, (ctypes.Structure,), {"_fields_": _struct_fields(body, constants, structs, tag)})
        return ""

    text = _STRUCT.sub(add_struct, text)
    decls = [" ".join(d.split()) for d in text.split(";")]
    if wrapped and decls[-1] == "}":
        decls[-1] = ""
    signatures = dict(_signature(d, structs) for d in decls if d)
    return constants, structs, signatures
