"""CPU-side checks of the binding that snac_amd/_lib.py derives from include/snac_hip.h (no GPU, no launch): the parser skips nothing
and guesses nothing, the host compiler lays the structs out as ctypes does, and the package keeps no hand copy of what it derives."""
import ctypes as C
import os
import re
import subprocess

import pytest

import helpers
from snac_amd import _lib

HEADER = os.path.join(helpers.ROOT, "include", "snac_hip.h")
STRUCT_NAMES = ("snac_sizes", "snac_env_hdr", "snac_env_desc", "snac_state", "snac_traj_info", "snac_rollout_record", "snac_node2d",
                "snac_node1d", "snac_node3d", "snac_uct_node")


def _stripped_header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_parser_skips_nothing():
    src = _stripped_header()
    functions = set(re.findall(r"\b(snac_[a-z0-9_]+)\s*\(", src))     # the loose regex of test_cabi_host._header_functions
    assert functions == set(_lib.PROTOTYPES) == set(_lib.EXPORTS) and len(functions) >= 89
    structs = re.findall(r"typedef\s+struct\s+(\w+)\s*\{", src)
    assert tuple(structs) == tuple(_lib.STRUCTS) and set(STRUCT_NAMES) <= set(structs)      # every one, in header order
    for name in re.findall(r"\b(SNAC_[A-Z0-9_]+)\s*=", src) + re.findall(r"#define\s+(SNAC_[A-Z0-9_]+)[ \t]+\S", src):
        assert name in _lib.CONSTANTS, name
        assert getattr(_lib, name[len("SNAC_"):]) == _lib.CONSTANTS[name]
    assert (_lib.ABI_VERSION, _lib.SNAC_OK, _lib.SUMS_SCRATCH_WORDS, _lib.TRAJ_INFO_WINDOWS) == (12, 0, 193, 64)
    for cls, name in ((_lib.Sizes, "snac_sizes"), (_lib.EnvDesc, "snac_env_desc"), (_lib.State, "snac_state"),
                      (_lib.RolloutRecord, "snac_rollout_record"), (_lib.TrajInfo, "snac_traj_info")):
        assert _lib.STRUCTS[name] is cls


def test_the_mapping_rules():
    """The rules of the binding on declarations whose types every rule meets: the fixed scalar table, POINTER(class) for the structs a
    caller constructs, c_void_p for every other pointer and for an array parameter, c_char_p only as a result."""
    vp, P = C.c_void_p, _lib.PROTOTYPES
    desc, st = C.POINTER(_lib.EnvDesc), C.POINTER(_lib.State)
    assert P["snac_step"] == (C.c_int, [desc, st, C.c_uint32, vp, vp, C.c_int, vp, vp, vp, vp])
    assert P["snac_step_scalar"] == (C.c_int, [desc, st, C.c_uint32, C.c_int32, C.c_int32, C.c_int, vp, vp, vp, vp])
    assert P["snac_rollout"] == (C.c_int, [desc, st, C.c_int32, C.c_uint32, vp, vp, C.c_int, vp, vp, vp, vp])
    assert P["snac_make_plans"][1] == [desc, st, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, vp, vp, vp]
    assert P["snac_prio_fill"][1] == [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, vp]
    assert P["snac_traj_alloc_ex"][1] == [C.c_size_t, C.c_int, C.c_size_t, vp, vp]            # void** out
    assert P["snac_traj_describe"][1] == [vp, C.POINTER(_lib.TrajInfo)] and P["snac_env_sizes"][1][2] == C.POINTER(_lib.Sizes)
    assert P["snac_rollout_rec"][1][10] == C.POINTER(_lib.RolloutRecord)
    assert P["snac_mailbox_stats"][1] == [vp, vp]                                            # const snac_mailbox*, uint32_t out[8]
    assert P["snac_nodes2d_pack"][1][4] == vp and P["snac_uct_select"][1][1] == vp            # snac_node2d*, snac_uct_node*
    assert P["snac_version"] == (C.c_int, []) and P["snac_last_error"] == (C.c_char_p, []) and P["snac_last_kernel"] == (C.c_char_p, [])
    assert P["snac_tuning"] == (C.c_int, [vp, C.c_int32])                                    # char* as a parameter
    assert P["snac_mailbox_row"] == (vp, [vp]) and P["snac_traj_reserved_bytes"] == (C.c_uint64, [])
    assert P["snac_replay_gather_nstep"][1][15] == C.c_double and len(P["snac_replay_gather_nstep"][1]) == 25
    L = _lib.lib()
    for name, (restype, argtypes) in P.items():
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    assert _lib.State._fields_[0] == ("hdr", vp) and _lib.STRUCTS["snac_node2d"]._fields_[0] == ("hdr", _lib.STRUCTS["snac_env_hdr"])
    assert _lib.EnvDesc(2, 1, 16, 4, 0, 0, 7, 9).env_id_base == 9                            # positional, in header order


@pytest.mark.parametrize("text", [
    "int snac_f(long a);",                                            # a type outside the table
    "int snac_f(unsigned int a);",
    "int snac_f(const snac_other* p);",                               # a pointer to a type nobody declared
    "snac_status snac_f(void);",
    "int snac_f(int32_t);",                                           # a parameter without a name
    "int snac_f(int32_t a, b);",
    "int snac_f(int (*fn)(int));",
    "typedef struct snac_s { int32_t a; unsigned b; } snac_s;",
    "typedef struct snac_s { int32_t a[SNAC_UNKNOWN]; } snac_s;",
    "typedef struct snac_s { int32_t a : 3; } snac_s;",
    "typedef struct snac_s { struct { int32_t a; } in; } snac_s;",
    "typedef struct snac_s snac_s; int snac_f(snac_s by_value);",
    "enum { SNAC_A };",
    "#define SNAC_A 1.5",
    "#define SNAC_A (7 / 2)",                                         # C and Python divide differently: not in the rule set
    "#define SNAC_A 0x10",
    "#define SNAC_A (1 +)",
    "#pragma pack(1)",
    "int snac_f(void); int snac_f(void);",
    "int other(void);",
    "int snac_f(void) { return 0; }",
    "int snac_f(void)",                                               # no semicolon: not fully consumed
])
def test_the_parser_never_guesses(text):
    with pytest.raises(_lib.SnacError, match="cannot bind"):
        _lib.parse_header(text)


def test_the_parser_reads_the_forms_the_header_uses():
    consts, structs, protos = _lib.parse_header("""
        #define SNAC_N (2 * 3 + 1)   /* a comment
                                        over two lines */
        enum { SNAC_A = -1, SNAC_B = 1 << 1 };
        typedef struct snac_in { int8_t a, b; int16_t c; } snac_in;
        typedef struct snac_out { snac_in head; const void* p; snac_in* q; float w[SNAC_N]; uint32_t z[4]; uint64_t big; } snac_out;
        typedef struct snac_opaque snac_opaque;
        const char* snac_name(void);
        double* snac_row(snac_opaque* o, const snac_out* s, snac_in** pp, uint32_t out[8], size_t n, float x);
    """)
    assert consts == {"SNAC_N": 7, "SNAC_A": -1, "SNAC_B": 2}
    assert [(n, t) for n, t in structs["snac_in"]._fields_] == [("a", C.c_int8), ("b", C.c_int8), ("c", C.c_int16)]
    out = structs["snac_out"]
    assert [n for n, _ in out._fields_] == ["head", "p", "q", "w", "z", "big"] and C.sizeof(out) == 4 + 4 + 8 + 8 + 28 + 16 + 4 + 8
    assert (out.w.offset, out.w.size, out.z.offset, out.big.offset) == (24, 28, 52, 72)
    vp = C.c_void_p
    assert protos == {"snac_name": (C.c_char_p, []), "snac_row": (vp, [vp, vp, vp, vp, C.c_size_t, C.c_float])}


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "INCLUDE", str(tmp_path))
    with pytest.raises(_lib.SnacError, match=re.escape(os.path.join(str(tmp_path), "snac_hip.h"))):
        _lib._header()


def test_the_compiler_agrees_with_the_parser(tmp_path):
    """A C program generated from the derived data prints sizeof and every offsetof of the ten structs and the value of every constant
    as the host compiler sees include/snac_hip.h: a field the parser dropped or mistyped shifts a size or a later offset."""
    lines, want = [], []
    for name, cls in _lib.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append("%s %d" % (name, C.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
            want.append("%s.%s %d %d" % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    for name, value in _lib.CONSTANTS.items():
        lines.append('printf("%s %%lld\\n", (long long)(%s));' % (name, name))
        want.append("%s %d" % (name, value))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "snac_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True, timeout=120)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(_lib.STRUCTS) >= 10 and len(_lib.CONSTANTS) >= 30 and len(want) >= 128
    assert got == want
    sizes = {n: C.sizeof(_lib.STRUCTS[n]) for n in STRUCT_NAMES}
    assert sizes == {"snac_sizes": 48, "snac_env_hdr": 16, "snac_env_desc": 64, "snac_state": 64, "snac_traj_info": 320,
                     "snac_rollout_record": 32, "snac_node2d": 128, "snac_node1d": 128, "snac_node3d": 896, "snac_uct_node": 256}


def test_record_sizes_and_word_offsets_come_from_the_structs():
    from snac_amd import nodes, uct

    assert (nodes.NodePool1D.WORDS, nodes.NodePool2D.WORDS, nodes.NodePool3D.WORDS, uct.WORDS) == (32, 32, 224, 64)
    assert (uct._CHILD, uct._CHILD_VISITS, uct._CHILD_VALUE) == (slice(0, 8), slice(8, 16), slice(16, 32))
    assert (uct._PARENT, uct._ACTION, uct._TERMINAL, uct._VISITS, uct._VALUE_SUM, uct._REWARD) == (32, 33, 34, 35, slice(36, 38), slice(38, 39))
    assert (uct._PRIOR, uct._NET_VALUE) == (48, 56)
    node = _lib.STRUCTS["snac_uct_node"]
    assert node.zero.offset + 4 * 9 == 4 * uct._PRIOR and node.zero.offset + 4 * 17 == 4 * uct._NET_VALUE     # zero[9], zero[17 .. 18]


def test_the_package_keeps_no_copy_of_what_it_derives():
    pkg = os.path.join(helpers.ROOT, "snac_amd")
    text = {f: open(os.path.join(pkg, f)).read() for f in sorted(os.listdir(pkg)) if f.endswith(".py")}
    assert not [f for f, s in text.items() if re.search(r"def _?ptr\b", s) and f != "_lib.py"]
    assert len(re.findall(r"def _?ptr\b", text["_lib.py"])) == 1
    assert "argtypes = [" not in text["_lib.py"] and "class Sizes" not in text["_lib.py"] and "EXPORTS = (\"" not in text["_lib.py"]
    # no integer literal indexes a word of self.stats in uct.py, first index or second, alone or in a slice
    assert not re.findall(r"stats(?:\[self\._roots\])?\[[^\]\n]*?(?:, ?|:)\d", text["uct.py"])
    assert not re.findall(r"\br\[:, *[\d:]", text["uct.py"])                              # nor a row gathered from it
    for f in ("nodes.py", "uct.py"):
        assigned = re.findall(r"^[ \t]*(?:\w+, )*WORDS(?:, \w+)* = (.*)$", text[f], flags=re.M)
        assert assigned and not [a for a in assigned if "None" not in a and "sizeof" not in a and "_words(" not in a], (f, assigned)
