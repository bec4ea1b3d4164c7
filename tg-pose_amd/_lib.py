"""ctypes binding of libtgpose_hip.so, derived from include/tgpose.h at import.

The header is the only place where the C ABI is written down: the argument structs (tgp_gemm_args -> GemmArgs, ...), SIGNATURES
and the constants (TGP_AUG_CROP -> AUG_CROP, ...) below are what _header.parse makes of it, so a declaration added there is
bound here with no further line.  tests/test_abi_cpu.py holds the result against what the C and C++ compilers make of the header.

There is NO fallback: if the library is missing or a call fails, this raises.  The product path
never routes through the CPU oracle or through torch ops for the hot layers.
"""
import ctypes
import os
import sys

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtgpose_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tgpose.h")

# CONSTANTS: name without TGP_ -> int; STRUCTS: C name -> ctypes.Structure; SIGNATURES: name -> (restype, argtypes), where a pointer
# to a struct is POINTER(that struct) and every other pointer, and tgp_stream_t, c_void_p.  Constants and structs are module attributes too.
with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, SIGNATURES = _header.parse(_f.read())
globals().update(CONSTANTS)
globals().update((cls.__name__, cls) for cls in STRUCTS.values())

PD_STATUS = {PD_ETETS: "TGP_PD_ETETS (tetrahedron / simplex storage)", PD_ECAVITY: "TGP_PD_ECAVITY (one insertion's cavity)",
             PD_EWALK: "TGP_PD_EWALK (point location did not end)", PD_EPAIRS: "TGP_PD_EPAIRS (more than PD_MAX_PAIRS pairs)",
             PD_ECOLUMNS: "TGP_PD_ECOLUMNS (H1 column storage)", PD_ERANGE: "TGP_PD_ERANGE (coordinate not finite or below the exact grid)",
             PD_EFLAT: "TGP_PD_EFLAT (fewer than 4 affinely independent points)", PD_EINTERNAL: "TGP_PD_EINTERNAL"}
# tgp_mesh_sample_args.status: the header names these two values in its comment only, they have no TGP_* macro
MESH_STATUS = {1: "the mesh's total area is not a positive finite number", 2: "the mesh index or the mesh's rows are outside the set"}
_lib = None


class TgpError(RuntimeError):
    pass


def lib():
    """Load the shared library once; raise loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TgpError(
                "tgpose_amd: %s not found. Build it with `python -m tgpose_amd.build` (hipcc, gfx950). "
                "There is no CPU/torch fallback for the HIP path." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if handle.tgp_version() != ABI_VERSION:
            raise TgpError("tgpose_amd: ABI version mismatch (%d != %d)" % (handle.tgp_version(), ABI_VERSION))
        if os.environ.get("TGP_TRACE", "0") != "0":
            # diagnosis: every entry point announces itself on stderr before it launches (with HIP_LAUNCH_BLOCKING=1 the last
            # name printed is the launch that faulted)
            class _Traced(object):
                def __init__(self, h):
                    self._h = h

                def __getattr__(self, name):
                    fn = getattr(self._h, name)

                    def call(*a):
                        sys.stderr.write("tgp: %s\n" % name)
                        sys.stderr.flush()
                        return fn(*a)
                    return call
            handle = _Traced(handle)
        _lib = handle
    return _lib


_ERR = {EINVAL: "TGP_EINVAL (bad pointer / size / stride / alignment)", EUNSUPPORTED: "TGP_EUNSUPPORTED (shape not supported)"}


def check(rc, what):
    if rc != 0:
        raise TgpError("%s failed: %s" % (what, _ERR.get(rc, "hipError_t %d" % rc)))
