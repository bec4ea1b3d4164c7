"""The C ABI in one place: what the C and C++ compilers make of include/tgpose.h against what tgpose_amd._lib derives from it.

Every struct field, constant and argument type is compared with the compiler's view, never with the parser's own (the lists of names
that the generated programs walk come from regular expressions of this file).  The parser's refusals are tested on small header texts."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from tests.util import ROOT

INCLUDE = os.path.join(ROOT, "include")
LETTER = {ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_float: "f", ctypes.c_double: "d", ctypes.c_uint32: "u", ctypes.c_uint64: "L",
          ctypes.c_void_p: "p"}
C_TYPES = (("int", "i"), ("int64_t", "l"), ("float", "f"), ("double", "d"), ("uint32_t", "u"), ("uint64_t", "L"))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "tgpose.h")).read(), flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(tgp_[a-z0-9_]+)\s*\(", _header())))


def _run(compiler, suffix, src):
    """compile (no library is linked) and run; -> the program's output lines, split into words"""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t" + suffix), "w") as f:
            f.write(src)
        subprocess.check_call(compiler + ["-I", INCLUDE, os.path.join(d, "t" + suffix), "-o", os.path.join(d, "t")])
        return [line.split() for line in subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()]


def _letter(ctype, struct_names):
    """the class of a ctypes type: one letter, or the C name of the struct a POINTER() points to"""
    return LETTER[ctype] if ctype in LETTER else struct_names[ctype._type_]


@pytest.fixture(scope="module")
def c_view():
    """one C program: sizeof of every struct; offset, size, alignment and type class of every field the binding holds; every TGP_*
    integer macro of the header"""
    from tgpose_amd import _lib
    generic = "_Generic((%s), " + ", ".join('%s: "%s"' % t for t in C_TYPES) + ', default: "p")'
    src = ['#include <stdio.h>\n#include <stddef.h>\n#include "tgpose.h"\nint main(void){']
    for cname, cls in _lib.STRUCTS.items():
        src.append('printf("S %s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            member = "((%s *)0)->%s" % (cname, f)
            src.append('printf("F %s %s %%zu %%zu %%zu %%s\\n", offsetof(%s, %s), sizeof(%s), __alignof__(%s), %s);'
                       % (cname, f, cname, f, member, member, generic % member))
    for macro in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(TGP_\w+)", _header(), flags=re.M):
        src.append('printf("C %s %%lld\\n", (long long)(%s));' % (macro, macro))
    out = _run(["gcc", "-std=c11"], ".c", "\n".join(src) + "return 0;}\n")
    return {kind: [w[1:] for w in out if w[0] == kind] for kind in "SFC"}


def test_every_struct_field_matches_the_compilers_layout(c_view):
    from tgpose_amd import _header as hp, _lib
    typedefs = re.findall(r"typedef\s+struct\b[^;{]*\{.*?\}\s*(\w+)\s*;", _header(), flags=re.S)
    assert len(typedefs) == len(re.findall(r"typedef\s+struct\b", _header())) >= 14
    assert sorted(_lib.STRUCTS) == sorted(typedefs)
    for cname, cls in _lib.STRUCTS.items():
        assert getattr(_lib, hp.class_name(cname)) is cls and issubclass(cls, ctypes.Structure)
    assert _lib.GemmArgs is _lib.STRUCTS["tgp_gemm_args"] and _lib.DecL1Args is _lib.STRUCTS["tgp_dec_l1_args"]
    assert _lib.PdArgs is _lib.STRUCTS["tgp_pd_args"] and _lib.RangerTensor is _lib.STRUCTS["tgp_ranger_tensor"]
    assert [(n, int(s)) for n, s in c_view["S"]] == [(n, ctypes.sizeof(c)) for n, c in _lib.STRUCTS.items()]
    want = []
    for cname, cls in _lib.STRUCTS.items():
        for f, t in cls._fields_:
            d = getattr(cls, f)
            want.append((cname, f, d.offset, d.size, "p" if hasattr(t, "_length_") else _letter(t, {})))      # an array decays in C
    assert [(c, f, int(o), int(s), k) for c, f, o, s, _, k in c_view["F"]] == want
    assert len(want) >= 311 and len(_lib.GemmArgs._fields_) == 61
    # the binding holds every field: the compiler's offsets leave no room between two fields, or behind the last, for one it missed
    end, align = {}, {}
    for cname, f, off, size, al, _ in c_view["F"]:
        off, size, al = int(off), int(size), int(al)
        assert off == -(-end.get(cname, 0) // al) * al, (cname, f)
        end[cname], align[cname] = off + size, max(al, align.get(cname, 1))
    for cname, size in c_view["S"]:
        assert int(size) == -(-end[cname] // align[cname]) * align[cname], cname


def test_every_constant_matches_the_compilers_value(c_view):
    from tgpose_amd import _lib
    consts = {name[len("TGP_"):]: int(v) for name, v in c_view["C"]}
    assert consts == _lib.CONSTANTS and len(consts) >= 46
    for name, v in consts.items():
        assert getattr(_lib, name) == v, name
    assert _lib.ABI_VERSION == 9 and _lib.EINVAL == -1 and _lib.EUNSUPPORTED == -2
    assert sorted(_lib.PD_STATUS) == list(range(1, 9)) and sorted(_lib._ERR) == [-2, -1]
    assert all(("TGP_PD_" + n[3:]) in _lib.PD_STATUS[v] for n, v in consts.items() if n.startswith("PD_E"))


def test_every_signature_matches_the_compilers_types():
    """one C++ program prints, for every declared function, the class of its return type and of each parameter (a pointer to one of the
    header's structs: that struct's name), deduced by a template from decltype(&fn): the functions are named in unevaluated
    operands only, so the program links without the library"""
    from tgpose_amd import _lib
    names = _declared_symbols()
    src = ['#include <cstdio>\n#include <type_traits>\n#include "tgpose.h"',
           'template <class T> struct L { static const char *s() { return std::is_pointer<T>::value ? "p" : "?"; } };',
           '#define CLASS(T, S) template <> struct L<T> { static const char *s() { return S; } };']
    src += ['CLASS(%s, "%s")' % t for t in C_TYPES]
    src += ['CLASS(%s%s *, "%s")' % (const, s, s) for s in _lib.STRUCTS for const in ("", "const ")]
    src += ['template <class R, class... A> void show(const char *name, R (*)(A...)) {',
            '    const char *a[] = {L<A>::s()..., 0};',
            '    printf("%s %s", name, L<R>::s());',
            '    for (const char **p = a; *p; ++p) printf(" %s", *p);',
            '    printf("\\n");', '}', 'int main() {']
    src += ['    show("%s", (decltype(&%s))0);' % (n, n) for n in names]
    out = _run(["g++", "-std=c++14"], ".cpp", "\n".join(src) + "\n    return 0;\n}\n")
    struct_names = {cls: cname for cname, cls in _lib.STRUCTS.items()}
    want = [[n, _letter(_lib.SIGNATURES[n][0], struct_names)] + [_letter(a, struct_names) for a in _lib.SIGNATURES[n][1]] for n in names]
    assert out == want
    assert not any("?" in line for line in out) and len(out) >= 157
    assert {w for line in out for w in line[2:]} - set("pilfduL") == set(_lib.STRUCTS)        # the struct pointers were told apart


def test_c_abi_exports_every_declared_symbol():
    from tgpose_amd import _lib
    names = _declared_symbols()
    assert len(names) >= 24
    assert sorted(_lib.SIGNATURES) == names            # the Python binding covers the header exactly
    handle = _lib.lib()                                # dlopen + symbol lookup for each; raises if one is missing
    for n in names:
        assert hasattr(handle, n)
    assert not hasattr(handle, "tgp_knn_feat_form")
    assert handle.tgp_version() == _lib.ABI_VERSION
    assert handle.tgp_knn_max_points() >= 1028 and handle.tgp_knn_max_k() >= 20


GOOD = """#define TGP_SLOTS 3
#define TGP_EBAD (-4)
typedef void *tgp_stream_t;
typedef struct tgp_toy_args {
    const float *src[TGP_SLOTS], *one; int n, m[2][TGP_SLOTS];
    uint64_t seed;
} tgp_toy_args;
int64_t tgp_toy_bytes(void);
int tgp_toy(const tgp_toy_args *args, int64_t rows,
            double scale, uint32_t *words, tgp_stream_t stream);
"""


def test_the_parser_refuses_what_it_does_not_understand():
    from tgpose_amd import _header as hp
    consts, structs, funcs = hp.parse(GOOD)
    toy = structs["tgp_toy_args"]
    assert consts == {"SLOTS": 3, "EBAD": -4} and toy.__name__ == "ToyArgs"
    assert [(f, getattr(toy, f).offset, getattr(toy, f).size) for f, _ in toy._fields_] == [
        ("src", 0, 24), ("one", 24, 8), ("n", 32, 4), ("m", 36, 24), ("seed", 64, 8)] and ctypes.sizeof(toy) == 72
    assert funcs == {"tgp_toy_bytes": (ctypes.c_int64, []),
                     "tgp_toy": (ctypes.c_int, [ctypes.POINTER(toy), ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p])}
    for good, bad, named in (("int64_t rows", "long rows", "`long`"),                       # an unknown parameter type
                             ("uint32_t *words", "size_t *words", "`size_t`"),               # ... also behind a pointer
                             ("src[TGP_SLOTS]", "src[TGP_SLOT]", "`TGP_SLOT`"),              # a struct field with an unknown array bound
                             ("uint64_t seed", "int (*seed)(int)", "(*seed)"),               # a field of a shape the header does not use
                             ("int64_t tgp_toy_bytes", "long tgp_toy_bytes", "long tgp_toy_bytes"),   # the function pattern misses it
                             ("TGP_EBAD (-4)", "TGP_EBAD (1 << 2)", "TGP_EBAD")):            # a #define that is no integer
        assert good in GOOD
        with pytest.raises(hp.HeaderError) as e:
            hp.parse(GOOD.replace(good, bad))
        assert named in str(e.value), (bad, str(e.value))              # the message names the offending text
