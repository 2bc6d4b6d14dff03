"""ctypes binding of libssd_hip.so.  include/ssd_hip.h is the only statement of the ABI: its constants, enumerators, structs
and prototypes are parsed here, once per process.  Fails loudly when the header or the library is absent, and on any
declaration the parser does not know."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# (SSD_HIP_LIB: development only -- another build of the library next to the default one, for same-box A/B runs)
LIB_PATH = os.path.join(HERE, os.environ.get("SSD_HIP_LIB", "libssd_hip.so"))
HEADER_PATH = os.path.join(HERE, "..", "include", "ssd_hip.h")

# The closed type map.  A pointer to a header struct is POINTER(its Structure), `const char*` is c_char_p, every other pointer
# is c_void_p: the header cannot say whether a `const double*` is a host array or a device address, and c_void_p takes
# ctypes arrays, integers and None alike.  _DEVICE_RECORDS: structs that live in device memory only (the library writes and
# reads arrays of them there); a pointer to one is an address like any tensor's, so c_void_p as well.
_DEVICE_RECORDS = {"ssd_augment_params"}
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64}


def _ctype(text, structs, where):
    """The ctypes type of a C type as written (`const float*`, `long long`, ...); `where` names the declaration in errors."""
    t = " ".join(re.sub(r"\bconst\b", " ", text).replace("*", " * ").split())
    if t.endswith("*"):
        base = t[:-1].strip()
        if base in structs and base not in _DEVICE_RECORDS:
            return ctypes.POINTER(structs[base])
        return ctypes.c_char_p if base == "char" else ctypes.c_void_p
    if t not in _SCALARS:
        raise TypeError("ssd_hip.h: no ctypes mapping for the type `%s` in `%s`" % (t, " ".join(where.split())))
    return _SCALARS[t]


def _enumerators(body):
    value = -1
    for item in filter(None, (s.strip() for s in body.split(","))):
        name, _, literal = (s.strip() for s in item.partition("="))
        value = int(literal, 0) if literal else value + 1
        yield name, value


def _fields(body, constants, structs, where):
    """_fields_ of a struct body: `int a, b;`, `int h[N], w[N];` and pointer members, N a literal or a #define."""
    declarator = r"\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*$"
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        base = ""
        for i, decl in enumerate(stmt.split(",")):
            m = re.match(declarator if i else r"(.*?)" + declarator, decl, re.S)
            if not m:
                raise TypeError("ssd_hip.h: cannot parse the member `%s` of %s" % (stmt, where))
            if i == 0:
                base = m.group(1)
            stars, name, bound = m.groups()[-3:]             # a `*` binds to its declarator, not to the comma list
            ctype = _ctype(base + stars, structs, "%s: %s" % (where, stmt))
            if bound:
                if not bound.isdigit() and bound not in constants:
                    raise TypeError("ssd_hip.h: unknown array bound `%s` in `%s` of %s" % (bound, stmt, where))
                ctype = ctype * (int(bound) if bound.isdigit() else constants[bound])
            yield name, ctype


def parse_header(text):
    """(constants, structs, signatures) of a C header in the style of ssd_hip.h: {name: int} for the integer #defines and
    every enumerator, {typedef name: ctypes.Structure class}, {function: (restype, [argtypes])}.  Anything it cannot type or
    does not recognise raises TypeError; nothing is guessed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {m.group(1): int(m.group(2), 0)
                 for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SSD_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)          # extern "C" { and its }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def enum(m):
        constants.update(_enumerators(m.group(1)))
        return " "

    text = re.sub(r"(?:typedef\s+)?enum\s*\w*\s*\{(.*?)\}\s*\w*\s*;", enum, text, flags=re.S)
    structs = {}

    def struct(m):
        cls = type(m.group(2), (ctypes.Structure,), {"__doc__": "%s of include/ssd_hip.h." % m.group(2)})
        cls._fields_ = list(_fields(m.group(1), constants, structs, m.group(2)))
        structs[m.group(2)] = cls
        return " "

    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.match(r"(.+?)\b(ssd_\w+)\s*\((.*)\)$", stmt, re.S)
        if not m:
            raise TypeError("ssd_hip.h: not a prototype, struct, enum or #define: `%s`" % " ".join(stmt.split()))
        params = [p.strip() for p in m.group(3).split(",")]
        params = [] if params == ["void"] else [re.match(r"(.*?)\w+$", p, re.S).group(1) for p in params]
        restype = _ctype(m.group(1), structs, stmt)
        signatures[m.group(2)] = (restype, [_ctype(p, structs, stmt) for p in params])
    return constants, structs, signatures


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError("include/ssd_hip.h is missing (%s): the ctypes binding is derived from it and there is no "
                           "hand-written copy to fall back to." % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return f.read()


CONSTANTS, STRUCTS, _SIGNATURES = parse_header(_read_header())
globals().update(CONSTANTS)         # SSD_OK, SSD_ERR_*, SSD_MAX_LEVELS, SSD_CHAIN_MAX_LAYERS, SSD_CHAIN_PACK_MAX, SSD_AUG_*, ...
PriorGrid = STRUCTS["ssd_prior_grid"]
HeadGrads = STRUCTS["ssd_head_grads"]                # the loss gradient as compact per-level pixel rows
HeadLayers = STRUCTS["ssd_head_layers"]              # operands and outputs of the head convolutions' backward pass
ChainLayer = STRUCTS["ssd_chain_layer"]              # one convolution of ssd_conv_chain
ChainPack = STRUCTS["ssd_chain_pack"]                # one filter tensor of ssd_chain_pack_weights
WgradItem = STRUCTS["ssd_wgrad_item"]                # one layer of ssd_conv2d_bwd_weight_batched
AugmentParams = STRUCTS["ssd_augment_params"]        # what ssd_augment_plan drew and applied for one image

_lib = None


def lib():
    """Load (once) and return the C-ABI library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libssd_hip.so is missing (%s): build it with `python ssd-object-detection_amd/build.py` "
                "or __graft_entry__.build(); there is no CPU fallback." % LIB_PATH)
        try:
            import torch  # noqa: F401  -- load torch's HIP runtime first so both share one libamdhip64
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, unsupported=None):
    """Map a C-ABI status to the exception type the reference raises at the same seam.  `unsupported`: the message of the
    NotImplementedError a wrapper raises instead where the library refuses a shape (SSD_ERR_UNSUPPORTED)."""
    if status == SSD_OK:
        return
    if unsupported is not None and status == SSD_ERR_UNSUPPORTED:
        raise NotImplementedError(unsupported)
    msg = lib().ssd_status_string(status).decode()
    if status == SSD_ERR_ASSERT:
        raise AssertionError(msg)
    if status in (SSD_ERR_VALUE, SSD_ERR_UNSUPPORTED):
        raise ValueError(msg)
    raise RuntimeError("ssd_hip: %s (status %d)" % (msg, status))
