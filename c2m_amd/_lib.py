"""ctypes binding of libc2m_hip.so; the signatures are parsed from include/c2m_hip.h.  There is NO fallback: if the
library is missing or a tensor is not on a HIP device, the op raises -- the product path never silently runs anything else."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("C2M_AMD_LIB") or os.path.join(_HERE, "lib", "libc2m_hip.so")   # override: tuning builds
HEADER = os.path.join(os.path.dirname(_HERE), "include", "c2m_hip.h")
_lib = None

# by-value parameter types a prototype may use; every pointer is a c_void_p (device addresses, ctypes arrays, None)
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "float": ctypes.c_float,
            "double": ctypes.c_double, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8}


def _parse_signatures(text):
    """{name: (restype, [argtypes])} of every `int|long c2m_*(...)` prototype in the text of include/c2m_hip.h.  The compiler
    holds the definitions in csrc/*.hip to the same prototypes (csrc/common.h includes the header), so this is the one place
    a signature is written.  Anything the table below cannot express raises, naming the function: nothing defaults to int."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    sigs = {}
    for ret, name, params in re.findall(r"\b(int|long)\s+(c2m_\w+)\s*\(([^()]*)\)\s*;", text):
        if name in sigs:
            raise ValueError(f"c2m_hip.h: {name} is declared twice")
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            tok = re.findall(r"\w+|\*", p)
            if "".join(tok) != "".join(p.split()) or len(tok) < 2 or tok[-1] in _SCALARS or tok[-1] in ("*", "const", "void"):
                raise ValueError(f"c2m_hip.h: {name}: cannot parse parameter {p.strip()!r} (want `type name`)")
            ty = [t for t in tok[:-1] if t != "const"]
            if "*" in ty[1:] and ty[0] != "*":
                args.append(ctypes.c_void_p)
            elif len(ty) == 1 and ty[0] in _SCALARS:
                args.append(_SCALARS[ty[0]])
            else:
                raise ValueError(f"c2m_hip.h: {name}: parameter {p.strip()!r} has no ctypes mapping "
                                 f"(by value: {', '.join(_SCALARS)}; or a pointer)")
        sigs[name] = (_SCALARS[ret], args)
    unparsed = sorted(set(re.findall(r"\b(c2m_\w+)\s*\(", text)) - set(sigs))
    if unparsed:
        raise ValueError(f"c2m_hip.h: cannot parse the prototype of {', '.join(unparsed)} (want `int|long name(type name, ...);`)")
    return sigs


with open(HEADER) as _f:
    _SIGS = _parse_signatures(_f.read())


GEOM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "c2m_geom.h")


class _Index(dict):
    """Enum of include/c2m_geom.h as attributes: G.M, G.PATCH_TY, ... (unknown names raise -- a typo is not index 0)."""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(f"c2m_geom.h defines no geom entry {k!r}") from None


def _parse_geom_header():
    with open(GEOM_HEADER) as f:
        text = f.read()
    version = int(re.search(r"#define\s+C2M_ABI_VERSION\s+(\d+)", text).group(1))
    conv = _Index((m.group(1), int(m.group(2))) for m in re.finditer(r"\bC2M_G_([A-Z0-9_]+)\s*=\s*(\d+)", text))
    wino = _Index((m.group(1), int(m.group(2))) for m in re.finditer(r"\bC2M_WG_([A-Z0-9_]+)\s*=\s*(\d+)", text))
    for tab in (conv, wino):          # every index once
        assert len(set(tab.values())) == len(tab), "c2m_geom.h: two names share an index"
    return version, conv, wino


ABI_VERSION, GEOM, WINO_GEOM = _parse_geom_header()


def declared_symbols():
    """Every function name declared in include/c2m_hip.h."""
    return sorted(_SIGS)


def lib():
    """Load (once) and return the library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"c2m_amd: HIP kernel library not found at {LIB_PATH}. Build it with "
                "`python -m c2m_amd.build` (needs hipcc); there is no CPU/PyTorch fallback for these ops.")
        # torch bundles its own HIP runtime (same SONAME as the system one).  It must be in the process BEFORE our
        # library is mapped so that both resolve to ONE runtime; the other order registers our kernels with a second
        # runtime that never sees torch's device context (every launch then fails with hipErrorNoDevice).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        if (L.c2m_abi_version(), L.c2m_geom_len(), L.c2m_wino_geom_len()) != (ABI_VERSION, GEOM.LEN, WINO_GEOM.LEN):
            raise RuntimeError(f"c2m_amd: {LIB_PATH} was built from another include/c2m_geom.h (library ABI "
                               f"{L.c2m_abi_version()}, geom {L.c2m_geom_len()} / {L.c2m_wino_geom_len()} entries; header ABI "
                               f"{ABI_VERSION}, {GEOM.LEN} / {WINO_GEOM.LEN}): rebuild with `python -m c2m_amd.build --force`")
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"c2m_amd: {what} failed with hipError_t={rc}")
