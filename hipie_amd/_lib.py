"""ctypes binding of libhipie_mi355.so (the C ABI of include/hipie_mi355.h).

The library is built in-tree (``make -C hipie_amd/csrc`` or ``__graft_entry__.build()``).  There is NO fallback: if the
shared object is missing or does not export a symbol, importing the op layer raises -- the product never silently runs a
PyTorch/CPU substitute for a hand-written kernel.

The prototypes and the integer ``#define``s are READ from the header at import: the header is the only description of an entry point.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIPIE_LIB_PATH: another build of the SAME ABI, for same-box A/B timing of a kernel change (tools/); the default is the in-tree library
LIB_PATH = os.environ.get("HIPIE_LIB_PATH") or os.path.join(_HERE, "csrc", "libhipie_mi355.so")
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "hipie_mi355.h")          # where csrc/Makefile finds it

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_l = ctypes.c_int64
c_f = ctypes.c_float
c_d = ctypes.c_double

_VALUE_TYPES = {"int": c_i, "int64_t": c_l, "float": c_f, "double": c_d}          # every pointer is a c_void_p
_RETURN_TYPES = {"int": c_i, "int64_t": c_l, "const char*": ctypes.c_char_p}


class HipieLibraryError(RuntimeError):
    pass


def parse_header(text):
    """(name -> argtypes, name -> restype, macro -> int) of a header in the style of include/hipie_mi355.h, in its order.  Every statement
    must be a prototype ``ret hipie_name(args);`` over the types above: anything else is refused, nothing is guessed."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {m.group(1): int(m.group(2), 0) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(HIPIE_\w+)[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', "", text, flags=re.M).strip()
    if text.endswith("}"):                                   # the brace that closes extern "C"
        text = text[:-1]
    signatures, restypes = {}, {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?)\s*\b(hipie_\w+)\s*\((.*)\)", stmt)
        if m is None:
            raise HipieLibraryError("hipie_mi355.h: not a prototype: `%s`" % stmt)
        ret, name, params = re.sub(r"\s*\*", "*", m.group(1)), m.group(2), m.group(3).strip()
        if ret not in _RETURN_TYPES or name in signatures:
            raise HipieLibraryError("hipie_mi355.h: unknown return type or repeated name in `%s`" % stmt)
        argtypes = []
        for param in ([] if params in ("", "void") else params.split(",")):
            words = [w for w in param.split() if w != "const"]
            if "*" in param:
                argtypes.append(c_p)
            elif len(words) == 2 and words[0] in _VALUE_TYPES:
                argtypes.append(_VALUE_TYPES[words[0]])
            else:
                raise HipieLibraryError("hipie_mi355.h: unknown parameter type `%s` in `%s`" % (param.strip(), stmt))
        signatures[name], restypes[name] = argtypes, _RETURN_TYPES[ret]
    return signatures, restypes, constants


with open(HEADER_PATH) as _f:
    SIGNATURES, RESTYPES, CONSTANTS = parse_header(_f.read())

_lib = None


def load():
    """dlopen the library once and set the prototypes; raises HipieLibraryError when it is absent, incomplete or of another ABI version."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipieLibraryError(
            "libhipie_mi355.so not found at %s -- build it with `make -C hipie_amd/csrc` (hipcc, gfx950). "
            "There is no PyTorch fallback for the hand-written kernels." % LIB_PATH)
    # PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's).  Import torch FIRST so that this library
    # binds to the HIP runtime instance torch has initialised: one runtime per process, shared streams and pointers.
    import torch  # noqa: F401
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # missing libamdhip64 etc.
        raise HipieLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise HipieLibraryError("%s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    if lib.hipie_version() != CONSTANTS["HIPIE_ABI_VERSION"]:
        raise HipieLibraryError("%s has ABI version %d, include/hipie_mi355.h has %d (stale build?)"
                                % (LIB_PATH, lib.hipie_version(), CONSTANTS["HIPIE_ABI_VERSION"]))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().hipie_last_error()
        raise HipieLibraryError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))
