"""ctypes binding of libsnac_hip.so.  There is no CPU fallback: if the HIP library is missing or a GPU is not available the
product raises.

include/snac_hip.h is the one statement of the ABI.  parse_header() reads it when this module is imported (no torch, no library) and
everything below comes from what it finds: the constants (ABI_VERSION, ENV_1D, ... are the header's SNAC_* names without the prefix),
a ctypes.Structure per struct (STRUCTS; Sizes, EnvDesc, State, RolloutRecord, TrajInfo and Mlp are the ones callers construct), EXPORTS, and
the restype / argtypes lib() sets on every entry point.  To bind a new entry point, struct or constant, declare it in the header: that is
all.  The parser knows only the header's own dialect and raises SnacError on anything else; it never guesses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNAC_HIP_LIB") or os.path.join(HERE, "libsnac_hip.so")  # override: A/B builds
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")


class SnacError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
            "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "float": C.c_float, "size_t": C.c_size_t}
_CLASS_NAMES = {"snac_sizes": "Sizes", "snac_env_desc": "EnvDesc", "snac_state": "State", "snac_rollout_record": "RolloutRecord",
                "snac_traj_info": "TrajInfo", "snac_mlp": "Mlp"}      # the structs callers construct: a parameter `T*` of one of them is POINTER(class)


def parse_header(text):
    """(constants, structs, prototypes) of a header written like include/snac_hip.h: {SNAC_NAME: int} of the enumerators and integer
    #defines, {struct name: ctypes.Structure} in header order, {function: (restype, argtypes)}.  Every pointer is c_void_p, except a
    parameter pointing to one of _CLASS_NAMES and a `const char*` result (c_char_p); an array parameter is a pointer."""
    consts, structs, protos = {}, {}, {}
    types = dict(_SCALARS, void=None, char=None)               # every type name so far; None: only pointers to it can be declared

    def bad(what):
        raise SnacError("include/snac_hip.h: cannot bind `%s` in `%s`" % (" ".join(what.split()), " ".join(decl.split())))

    def integer(expr):
        text = re.sub(r"SNAC_\w+", lambda m: str(consts[m.group()]) if m.group() in consts else bad(expr), expr)
        if not re.fullmatch(r"[-+*<>|&() \d]*\d[) ]*", text):  # decimal digits, + - * << >> | & and parentheses only
            bad(expr)
        try:
            return int(eval(text, {"__builtins__": {}}))
        except (SyntaxError, TypeError):
            bad(expr)

    typed = re.compile(r"(?:const )?(\w+)\b(.*)").fullmatch                        # `type` and its declarators
    declarator = re.compile(r" ?(\**) ?(\w+) ?(?:\[ ?(\w+) ?\])?").fullmatch          # `*name[n]`

    def declare(part, field):
        """[(name, ctype)] of `type a, *b, c[n]`: the fields of a struct, or (field False) a parameter or a function's name and result."""
        base, rest = (typed(part) or bad(part)).groups()
        if base not in types:
            bad(part)
        out = []
        for d in rest.split(","):
            stars, name, dim = (declarator(d) or bad(part)).groups()
            if stars or (dim and not field):
                t = C.POINTER(structs[base]) if base in _CLASS_NAMES and stars == "*" and not (dim or field) else C.c_void_p
                if dim and field:                                    # a field `const float* w[4]`: an array of pointers
                    t = t * integer(dim)
            else:
                t = types[base] or bad(part)
                if dim:
                    t = t * integer(dim)
            out.append((name, t))
        return out

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^#ifdef __cplusplus\n.*\n#endif$", "", text, flags=re.M)       # extern "C" { and its }
    for decl in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = re.fullmatch(r"#define (SNAC_\w+) (.+)", " ".join(decl.split()))
        if m:
            consts[m.group(1)] = integer(m.group(2))
        elif not re.fullmatch(r"#(ifndef \w+|define \w+|include <\w+\.h>|endif)", decl.strip()):
            bad(decl)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    one = re.compile(r"\s*([^;{}]*(?:\{[^{}]*\}[^;{}]*)?);")             # a declaration, with at most one { } body
    pos = 0
    while text[pos:].strip():
        decl = text[pos:pos + 120]
        m = one.match(text, pos) or bad("what follows")
        pos, decl = m.end(), " ".join(m.group(1).split())
        enum = re.fullmatch(r"(?:typedef )?enum(?: \w+)? \{(.*)\}(?: \w+)?", decl)
        struct = re.fullmatch(r"typedef struct (\w+) (?:\{(.*)\} )?\1", decl)
        if enum:
            for e in enum.group(1).split(","):
                name, value = (re.fullmatch(r" ?(SNAC_\w+) = (.+)", e) or bad(decl)).groups()
                consts[name] = integer(value)
        elif struct and struct.group(2) is None:
            types[struct.group(1)] = None                            # typedef struct snac_mailbox snac_mailbox;
        elif struct:
            name, body = struct.groups()
            fields = [f for part in body.split(";") if part.strip() for f in declare(part.strip(), True)]
            types[name] = structs[name] = type(_CLASS_NAMES.get(name, name), (C.Structure,), {"_fields_": fields})
        else:
            result, params = (re.fullmatch(r"([^()]+)\((.*)\)", decl) or bad(decl)).groups()
            (name, res), = declare(result.strip(), False)
            if name in protos or not name.startswith("snac_"):
                bad(decl)
            if result.startswith("const char*"):
                res = C.c_char_p
            args = [] if params.strip() == "void" else [declare(a.strip(), False) for a in params.split(",")]
            protos[name] = (res, [t for (_, t), in args])
    return consts, structs, protos


def _header():
    path = os.path.join(INCLUDE, "snac_hip.h")
    try:
        with open(path) as fh:
            return fh.read()
    except OSError as e:
        raise SnacError("the header of the C ABI is missing: %s" % path) from e


CONSTANTS, STRUCTS, PROTOTYPES = parse_header(_header())
globals().update({k[len("SNAC_"):]: v for k, v in CONSTANTS.items()})      # ABI_VERSION, ENV_1D .. TAIL_RECORD, SUMS_SCRATCH_WORDS, ...
SNAC_OK = CONSTANTS["SNAC_OK"]
Sizes, EnvDesc, State, RolloutRecord, TrajInfo, Mlp = (STRUCTS[n] for n in _CLASS_NAMES)
EXPORTS = tuple(PROTOTYPES)


def ptr(t):
    """A tensor's address as a pointer argument; None stays None (NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def build(force=False):
    """Compile libsnac_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    src = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".inc")) or f == "Makefile"]
    src.append(os.path.join(INCLUDE, "snac_hip.h"))
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in src):
        # one object per translation unit, compiled in parallel (snac_amd/csrc/Makefile: `fast`)
        jobs = str(max(1, min(8, os.cpu_count() or 1)))
        subprocess.check_call(["make", "-s", "-C", CSRC, "JOBS=" + jobs] + (["clean", "fast"] if force else ["fast"]))
    return LIB_PATH


def kernel_source_sha16():
    """First 16 hex digits of the sha256 over the headline kernel's source (snac_dev.h + k_roll2d.hip): what profiles/traffic.json
    is stamped with, so that bench.py reports counter traffic only for the kernel source the counters were taken with."""
    import hashlib

    h = hashlib.sha256()
    for f in ("snac_dev.h", "k_roll2d.hip"):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SnacError("libsnac_hip.so is not built (%s); run __graft_entry__.build() or `make -C snac_amd/csrc`. "
                            "There is no CPU fallback." % LIB_PATH)
        # torch first: libsnac_hip.so needs libamdhip64.so.7 and must bind to the HIP runtime that PyTorch-ROCm
        # bundles (same SONAME) -- loading the system copy beside it would put two runtimes in one process.
        import torch  # noqa: F401

        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():        # a symbol the library lacks raises here
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.snac_version() != CONSTANTS["SNAC_ABI_VERSION"]:
            raise SnacError("libsnac_hip.so ABI version mismatch")
        _lib = L
    return _lib


def tuning():
    """The library's dispatch table as {environment variable: (effective value, what it decides)} (snac_tuning)."""
    buf = C.create_string_buffer(16384)
    check(lib().snac_tuning(buf, len(buf)))
    out = {}
    for ln in buf.value.decode().splitlines():
        kv, _, what = ln.partition("  # ")
        k, _, v = kv.partition("=")
        out[k] = (int(v), what)
    return out


def check(rc):
    if rc != SNAC_OK:
        raise SnacError("libsnac_hip: %s (code %d)" % (lib().snac_last_error().decode(), rc))


def action_cdf(probs, num_actions):
    """Thresholds of the counter RNG's action draw (include/snac_hip.h, "Counter RNG") for `num_actions` weights: finite,
    non-negative, with a positive sum.  C = the float64 cumulative sum of probs / sum(probs), in order;
    cdf[j] = min(65536, ceil(65536 * C[j])) for j < num_actions - 1 (uint32 array)."""
    p = np.asarray(probs, dtype=np.float64)
    if p.shape != (num_actions,):
        raise ValueError("action_probs must hold %d weights, one per action" % num_actions)
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        raise ValueError("action_probs must be finite and non-negative")
    total = p.sum()
    if not total > 0:
        raise ValueError("action_probs must have a positive sum")
    c = np.cumsum(p / total)[:-1]
    return np.minimum(65536.0, np.ceil(65536.0 * c)).astype(np.uint32)


def action_dist(num_actions, cdf):
    """snac_action_dist: the handle (>= 1) of the thresholds `cdf` for `num_actions` actions (the same table, the same handle)."""
    if len(cdf) != num_actions - 1:
        raise ValueError("cdf must hold num_actions - 1 thresholds")
    arr = (C.c_uint32 * max(1, num_actions - 1))(*[int(x) for x in cdf])
    h = C.c_int32(0)
    check(lib().snac_action_dist(int(num_actions), arr, C.byref(h)))
    return h.value


def env_sizes(kind, dynamic):
    s = Sizes()
    check(lib().snac_env_sizes(kind, int(bool(dynamic)), C.byref(s)))
    return s
