"""ctypes binding of libscan_hip.so (the C ABI declared in include/scan_hip.h).

The library is the product: there is no CPU or PyTorch fallback.  ``lib()``
raises if the shared object is missing and every compute entry point raises
``RuntimeError`` (with ``scan_last_error()``) on a non-zero return, mirroring
the reference's AT_ASSERTM/AT_ERROR -> RuntimeError behaviour
(reference fcos_core/csrc/nms.h:10-28, csrc/SigmoidFocalLoss.h:10-41).

The header is the only statement of the ABI: ``SIGNATURES``, the ``Structure`` classes and the ``SCAN_*`` constants below are
parsed from it at import, and text the parser does not understand is an error, never a guess.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCAN_HIP_LIB: an alternative build of the same library (timing experiments, see csrc/Makefile); default = the product
LIB_PATH = os.environ.get("SCAN_HIP_LIB") or os.path.join(_HERE, "libscan_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "scan_hip.h")  # where csrc/Makefile finds it: ../../include

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(_SCALARS) | {"void", "uint8_t"}  # what a c_void_p parameter or field may point to
# header struct -> Python class; everything else about the classes comes from the header
_STRUCTS = {"scan_pyramid_t": "PyramidDesc", "scan_sgd_segment_t": "SgdSegment", "scan_cka_branch_t": "CkaBranch",
            "scan_level_t": "LevelDesc", "scan_conv_plan_t": "ConvPlan", "scan_conv_wgrad_plan_t": "WgradPlan",
            "scan_groupnorm_plan_t": "GroupNormPlan"}


def _parse_header(text, struct_names):
    """C header text -> (constants {SCAN_X: int}, structs {python name: Structure class}, signatures {scan_name: (restype,
    argtypes)}).  Understands what include/scan_hip.h is written in -- integer #defines, ``typedef struct { ... } name;`` and
    ``type scan_name(args);`` over the types of _SCALARS, ``const char*``, the structs of ``struct_names`` and pointers --
    and raises ValueError naming the text for anything else."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, structs, by_c_name, sigs = {}, {}, {}, {}

    def integer(expr):
        expr = re.sub(r"\bSCAN_\w+", lambda m: str(consts[m.group()]) if m.group() in consts else m.group(), expr)
        if not re.fullmatch(r"[0-9\s()+*-]+", expr):
            raise ValueError("scan_hip.h: not an integer expression: %r" % expr)
        return int(eval(expr, {"__builtins__": {}}))  # digits, parentheses, + - * only

    def ctype(decl, field=False):
        """the ctypes class of ``[const] base [*...] [name]``"""
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(?:\b\w+)?", decl.strip())
        base, depth = (m.group(1), m.group(2).count("*")) if m else (None, 0)
        if depth == 0 and base in _SCALARS:
            return _SCALARS[base]
        if depth == 1 and base == "char" and not field:
            return ctypes.c_char_p
        if depth == 1 and base in by_c_name and not field:
            return ctypes.POINTER(by_c_name[base])
        if depth >= 1 and (base in _POINTEES or base in by_c_name):
            return ctypes.c_void_p
        raise ValueError("scan_hip.h: unknown type in %r" % decl.strip())

    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SCAN_\w+)[ \t]+(\S.*)$", text, re.M):
        consts[name] = integer(expr)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "")

    def struct(m):
        fields = []
        for line in filter(None, (s.strip() for s in m.group(1).split(";"))):
            first, *more = line.split(",")  # "int32_t O, Cs_w": the first declarator carries the type
            base = re.sub(r"\w+\s*(\[.*\])?$", "", first.strip())
            for d in [first] + [base + s for s in more]:
                m1 = re.fullmatch(r"(.*?)(\w+)\s*(?:\[(.*)\])?", d.strip())
                if m1 is None:
                    raise ValueError("scan_hip.h: cannot split the field %r of %s" % (line, m.group(2)))
                t = ctype(m1.group(1) + m1.group(2), field=True)
                fields.append((m1.group(2), t * integer(m1.group(3)) if m1.group(3) else t))
        if m.group(2) in struct_names:
            cls = type(struct_names[m.group(2)], (ctypes.Structure,), {"_fields_": fields, "__doc__": m.group(2)})
            structs[cls.__name__] = by_c_name[m.group(2)] = cls
        return ""

    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    missing = sorted(set(struct_names) - set(by_c_name))
    if missing:
        raise ValueError("scan_hip.h: no typedef struct { ... } %s" % ", ".join(missing))
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(scan_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if m is None:
            if stmt == "}":  # closes extern "C"
                continue
            raise ValueError("scan_hip.h: cannot split the declaration %r" % stmt)
        args = m.group(3).strip()
        sigs[m.group(2)] = (ctype(m.group(1)), [] if args == "void" else [ctype(a) for a in args.split(",")])
    return consts, structs, sigs


if not os.path.exists(HEADER_PATH):
    raise RuntimeError("scan_amd: %s is missing -- the ctypes binding is derived from it" % os.path.normpath(HEADER_PATH))
with open(HEADER_PATH) as _f:
    _consts, _structs, SIGNATURES = _parse_header(_f.read(), _STRUCTS)  # SIGNATURES: name -> (restype, argtypes)
# PyramidDesc, SgdSegment, CkaBranch, LevelDesc, ConvPlan, WgradPlan, GroupNormPlan; every SCAN_X as X (MAX_LEVELS,
# TUNE_UNKNOWN, NMS_PANEL, NMS_MAX, CONV_*, WGRAD_*, GN_*, PACK_MAX_LEVELS, SGD_MAX_SEGMENTS, CKA_MAX_CLASSES, ...)
globals().update(_structs)
globals().update({k[len("SCAN_"):]: v for k, v in _consts.items()})

_lib = None


def lib():
    """Load libscan_hip.so; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "scan_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
        # PyTorch-ROCm ships its own libamdhip64; load it first so this library binds to the SAME HIP runtime
        # (two runtimes in one process do not see each other's device context)
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        # SCAN_TUNE="key=value,key=value": launch-selection knobs for A/B measurements (scan_tune, include/scan_hip.h)
        for kv in filter(None, os.environ.get("SCAN_TUNE", "").split(",")):
            key, _, val = kv.partition("=")
            if L.scan_tune(key.strip().encode(), int(val)) == TUNE_UNKNOWN:  # noqa: F821 (SCAN_TUNE_UNKNOWN of the header)
                raise RuntimeError("SCAN_TUNE: unknown key %r" % key)
        _lib = L
    return _lib


def tune_state():
    """{knob: (value, default)} of every scan_tune knob of the loaded library"""
    L, out, i = lib(), {}, 0
    while True:
        k = L.scan_tune_key(i)
        if k is None:
            return out
        out[k.decode()] = (L.scan_tune_get(k), L.scan_tune_default(k))
        i += 1


def lib_identity():
    """what a measurement was taken with: the library file (basename, sha1 of its bytes, whether it is the product library
    and not an alternative build selected by SCAN_HIP_LIB) and every scan_tune knob that is off its default"""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        sha = hashlib.sha1(f.read()).hexdigest()
    product = os.path.realpath(LIB_PATH) == os.path.realpath(os.path.join(_HERE, "libscan_hip.so"))
    return {"lib": os.path.basename(LIB_PATH), "lib_sha1": sha, "product_library": product,
            "scan_tune_non_default": {k: v for k, (v, d) in tune_state().items() if v != d}}


def call(name, *args):
    """Call a status-returning entry point; raise RuntimeError on failure."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (name, rc, lib().scan_last_error().decode()))


def query(name, *args):
    return getattr(lib(), name)(*args)
