"""Reads include/tgpose.h into ctypes: the header is the only place where the C ABI is written down.

parse(text) understands exactly what the header uses -- `#define TGP_X <integer>`, `typedef struct [tag] { ... } name;` and
`int | int64_t tgp_name(...);` in the header's one regular style -- and raises HeaderError, naming the text, for anything else:
a declaration that is skipped here would be called with the wrong argument types.
"""
import ctypes
import re

# types passed by value; a pointer may point to these, to void, to the narrower integers or to a struct of the header
VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
         "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
POINTEE = set(VALUE) | {"void", "int32_t", "uint8_t", "uint16_t"}
STREAM = "tgp_stream_t"

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+TGP_(\w+)(.*)$", re.M)
_INTEGER = re.compile(r"\s+(\(\s*[-+]?\d+\s*\)|[-+]?\d+)\s*")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
_FUNCTION = re.compile(r"(int|int64_t)\s+(tgp_[a-z0-9_]+)\s*\((.*)\)", re.S)
_DECLARATION = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\**)(\w+)((?:\[\w+\])*)")


class HeaderError(ValueError):
    pass


def class_name(c_name):
    """tgp_conv_max_fused_args -> ConvMaxFusedArgs"""
    return "".join(part.capitalize() for part in c_name[len("tgp_"):].split("_"))


def _declarators(decl, known, what):
    """`const float *R, *t` -> [("float", 1, "R", []), ("float", 1, "t", [])]; every type name must be known"""
    m = _DECLARATION.fullmatch(" ".join(decl.split()))
    if not m:
        raise HeaderError("%s: cannot parse `%s`" % (what, decl.strip()))
    base, out = m.group(1), []
    for d in m.group(2).split(","):
        dm = _DECLARATOR.fullmatch(d.replace(" ", ""))
        if not dm:
            raise HeaderError("%s: cannot parse `%s`" % (what, decl.strip()))
        stars = len(dm.group(1))
        if base not in (POINTEE | known if stars else set(VALUE) | {STREAM}):
            raise HeaderError("%s: unknown type `%s` in `%s`" % (what, base, decl.strip()))
        out.append((base, stars, dm.group(2), re.findall(r"\[(\w+)\]", dm.group(3))))
    return out


def parse(text):
    """-> (constants {name without TGP_: int}, structs {C name: ctypes.Structure class}, functions {name: (restype, argtypes)})"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = set(re.findall(r"\b(tgp_[a-z0-9_]+)\s*\(", text))

    constants = {}
    for name, value in _DEFINE.findall(text):
        if not _INTEGER.fullmatch(value):
            raise HeaderError("#define TGP_%s: `%s` is not an integer" % (name, value.strip()))
        constants[name] = int(value.strip(" \t()"))

    structs = {}
    for body, c_name in _STRUCT.findall(text):
        fields = []
        for decl in filter(str.strip, body.split(";")):
            for base, stars, name, bounds in _declarators(decl, set(structs), "struct " + c_name):
                ctype = ctypes.c_void_p if stars or base == STREAM else VALUE[base]
                for bound in reversed(bounds):
                    if not (bound.isdigit() or bound[:4] == "TGP_" and bound[4:] in constants):
                        raise HeaderError("struct %s: unknown array bound `%s` in `%s`" % (c_name, bound, decl.strip()))
                    ctype = ctype * (int(bound) if bound.isdigit() else constants[bound[4:]])
                fields.append((name, ctype))
        structs[c_name] = type(class_name(c_name), (ctypes.Structure,),
                               {"_fields_": fields, "__doc__": "struct %s (include/tgpose.h)" % c_name})

    # what is left are the preprocessor lines, the stream typedef, the extern "C" braces and one function per statement
    rest = re.sub(r'^[ \t]*#.*$|typedef\s+void\s*\*\s*%s\s*;|extern\s+"C"\s*\{|^\}[ \t]*$' % STREAM, "", _STRUCT.sub("", text), flags=re.M)
    functions = {}
    for stmt in filter(str.strip, rest.split(";")):
        m = _FUNCTION.fullmatch(stmt.strip())
        if not m:
            raise HeaderError("cannot parse `%s`" % " ".join(stmt.split()))
        argtypes = []
        for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            (base, stars, _, bounds), = _declarators(param, set(structs), m.group(2))
            if bounds or stars > 1 and base in structs:
                raise HeaderError("%s: cannot parse `%s`" % (m.group(2), param.strip()))
            argtypes.append(ctypes.POINTER(structs[base]) if base in structs else
                            ctypes.c_void_p if stars or base == STREAM else VALUE[base])
        functions[m.group(2)] = (VALUE[m.group(1)], argtypes)
    if set(functions) != declared:
        raise HeaderError("declarations not understood: %s" % ", ".join(sorted(declared ^ set(functions))))
    return constants, structs, functions
