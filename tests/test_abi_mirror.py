"""CPU: slide_amd/abi.py (and the four structs of slide_amd/experiments/resident.py) against the C headers.

The headers are the contract; Python restates it once.  A C probe generated from the header TEXT is compiled with the host C
compiler and prints sizeof of every struct, offsetof / size of every field and the value of every SLIDE_* enumerator and
#define; every SLIDE_API declaration is parsed for its return and parameter types.  Each is compared with the ctypes side in both
directions (a name on one side only is a failure), and the comparison functions are run on deliberately wrong Python copies to
show that they report.  No device is needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO
from slide_amd import _lib, abi, build
from slide_amd.experiments import resident

INCLUDE = os.path.join(REPO, "include")
PRODUCT_HEADERS = ("slide_hip.h", "slide_engine.h", "slide_train.h")
RESIDENT_HEADER = "experiments/slide_resident.h"


def _text(header):
    src = open(os.path.join(INCLUDE, header)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


# ------------------------------------------------------------------------------------------------ what the header text names
def header_structs(header):
    """{struct: [field, ...]} in declaration order"""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _text(header), flags=re.S):
        assert m.group(1) == m.group(3)
        fields = []
        for decl in m.group(2).split(";"):
            for part in decl.split(","):  # `const float *sum, *sq` declares two
                f = re.search(r"(\w+)\s*(?:\[\s*\d+\s*\])?\s*$", part.strip())
                if f:
                    fields.append(f.group(1))
        out[m.group(1)] = fields
    return out


def header_constants(header):
    """names of the SLIDE_* enumerators and of the SLIDE_* macros that have a value (not the include guard, not SLIDE_API)"""
    src = _text(header)
    names = [e.split("=")[0].strip() for m in re.finditer(r"\benum\s*\{(.*?)\}", src, flags=re.S) for e in m.group(1).split(",")
             if e.strip()]
    names += [m.group(1) for m in re.finditer(r"(?m)^\s*#\s*define\s+(SLIDE_\w+)[ \t]+\S", src) if m.group(1) != "SLIDE_API"]
    assert all(n.startswith("SLIDE_") for n in names), names
    return names


def _ctype_of(c_type):
    """the issue's rule: every pointer and slide_stream_t -> c_void_p, const char * as a RETURN -> c_char_p (handled by the caller)"""
    t = " ".join(w for w in c_type.replace("*", " * ").split() if w != "const")
    if "*" in t or t == "slide_stream_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}[t]


def header_prototypes(header):
    """{function: (restype, (argtype, ...))} of every SLIDE_API declaration"""
    out = {}
    for m in re.finditer(r"SLIDE_API\s+([^;()]+?)\b(\w+)\s*\(([^;{}]*)\)\s*;", re.sub(r"(?m)^\s*#.*$", "", _text(header))):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        restype = ctypes.c_char_p if ret == "const char *" else _ctype_of(ret)
        args = []
        if params != "void":
            for p in params.split(","):
                args.append(_ctype_of(re.sub(r"\w+\s*$", "", p.strip())))  # (drop the parameter's name)
        out[name] = (restype, tuple(args))
    return out


# ------------------------------------------------------------------------------------------------ what the C compiler says
@pytest.fixture(scope="module")
def c_facts(tmp_path_factory):
    """({struct: (sizeof, {field: (offset, size)})}, {constant: value}) of all four headers, from a compiled probe"""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a host C compiler is needed"
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + ['#include "%s"' % h for h in PRODUCT_HEADERS + (RESIDENT_HEADER,)]
    lines.append("int main(void) {")
    for h in PRODUCT_HEADERS + (RESIDENT_HEADER,):
        for s, fields in header_structs(h).items():
            lines.append('  printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
            for f in fields:
                lines.append('  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
        for c in header_constants(h):
            lines.append('  printf("C %s %%lld\\n", (long long)(%s));' % (c, c))
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_probe")
    (d / "probe.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, "-o", str(d / "probe"), str(d / "probe.c")], check=True)
    structs, consts = {}, {}
    for ln in subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = ln.split()
        if w and w[0] == "S":
            structs[w[1]] = (int(w[2]), {})
        elif w and w[0] == "F":
            structs[w[1]][1][w[2]] = (int(w[3]), int(w[4]))
        elif w and w[0] == "C":
            consts[w[1]] = int(w[2])
    return structs, consts


# ------------------------------------------------------------------------------------------------ the comparisons
def _py_structs(module, skip=()):
    return {n: c for n, c in vars(module).items() if isinstance(c, type) and issubclass(c, ctypes.Structure)
            and c is not ctypes.Structure and c.__module__ == module.__name__ and n not in skip}


def struct_mismatches(c_structs, py_structs):
    """c_structs {name: (sizeof, {field: (offset, size)})} against ctypes classes {name: class}; -> list of messages"""
    bad = ["struct %s is on one side only" % n for n in sorted(set(c_structs) ^ set(py_structs))]
    for n in sorted(set(c_structs) & set(py_structs)):
        (size, fields), cls = c_structs[n], py_structs[n]
        py_fields = [f[0] for f in cls._fields_]
        if ctypes.sizeof(cls) != size:
            bad.append("sizeof(%s): C %d, ctypes %d" % (n, size, ctypes.sizeof(cls)))
        if py_fields != list(fields):  # (dicts keep the header's order)
            bad.append("%s: fields differ in name or order: C %s, ctypes %s" % (n, list(fields), py_fields))
        for f in set(fields) & set(py_fields):
            d = getattr(cls, f)
            if (d.offset, d.size) != fields[f]:
                bad.append("%s.%s: (offset, size) C %s, ctypes %s" % (n, f, fields[f], (d.offset, d.size)))
    return bad


def constant_mismatches(c_consts, py_consts):
    """{SLIDE_X: value} of the compiled headers against {X: value} of Python; -> list of messages"""
    want = {n[len("SLIDE_"):]: v for n, v in c_consts.items()}
    bad = ["constant %s is on one side only" % n for n in sorted(set(want) ^ set(py_consts))]
    return bad + ["%s: C %d, Python %r" % (n, want[n], py_consts[n]) for n in sorted(set(want) & set(py_consts)) if want[n] != py_consts[n]]


def prototype_mismatches(c_protos, py_protos):
    bad = ["function %s is on one side only" % n for n in sorted(set(c_protos) ^ set(py_protos))]
    for n in sorted(set(c_protos) & set(py_protos)):
        (cr, ca), (pr, pa) = c_protos[n], py_protos[n]
        if cr is not pr:
            bad.append("%s: return type C %s, Python %s" % (n, cr.__name__, pr.__name__))
        if len(ca) != len(pa):
            bad.append("%s: %d parameters in C, %d in Python" % (n, len(ca), len(pa)))
        bad += ["%s: parameter %d C %s, Python %s" % (n, k, a.__name__, b.__name__) for k, (a, b) in enumerate(zip(ca, pa)) if a is not b]
    return bad


def _product(d, names_of):
    keep = set(n for h in PRODUCT_HEADERS for n in names_of(h))
    return {n: v for n, v in d.items() if n in keep}, {n: v for n, v in d.items() if n not in keep}


def _abi_constants():
    """abi's restatement of the header constants: every OP_ / EPI_ / F_ / PREC_ integer (ST_EXPERIMENT, the GROUP_ / GN_ / POOL_ /
    GEMM_ / TAIL_ flag sets and CHAMFER_TERM have no header name: abi.py says so)"""
    return {n: v for n, v in vars(abi).items() if re.match(r"(OP|EPI|F|PREC)_", n) and isinstance(v, int)}


def _resident_constants():
    return {n: v for n, v in vars(resident).items() if re.match(r"R[SFO]?_", n) and isinstance(v, int)}


# ------------------------------------------------------------------------------------------------ the tests
def test_the_parsers_see_the_headers():
    """(a parser that silently finds nothing would make every comparison below pass)"""
    assert list(header_structs("slide_engine.h")) == ["SlideEpi", "SlideGnFin", "SlidePrepCopy", "SlideChainLayer", "SlideHeadArgs",
                                                      "SlidePointChainArgs", "SlideOp"]
    assert header_structs("slide_engine.h")["SlideOp"] == ["kind", "i", "f", "p"]
    assert header_structs("slide_engine.h")["SlideGnFin"][:5] == ["sum", "sq", "gid", "gstart", "gend"]
    assert list(header_structs(RESIDENT_HEADER)) == ["RIn", "ROp", "RStrip", "RArgs"]
    consts = header_constants("slide_engine.h")
    assert {"SLIDE_OP_GEMM", "SLIDE_OP_ROWS_GN_JOINT", "SLIDE_EPI_PACKED_VECS", "SLIDE_F_OUT_FM", "SLIDE_PREC_SPLIT"} <= set(consts)
    assert "SLIDE_ENGINE_H" not in consts and "SLIDE_API" not in consts and len(consts) == len(set(consts)) >= 49
    protos = header_prototypes("slide_train.h")
    assert protos["slide_col_sums"] == (ctypes.c_int, (ctypes.c_longlong, ctypes.c_int) + (ctypes.c_void_p,) * 4)
    assert header_prototypes("slide_hip.h")["slide_hip_version"] == (ctypes.c_char_p, ())
    assert header_prototypes("slide_hip.h")["query_ball_point_kernel_wrapper"][1][3] is ctypes.c_float


def test_struct_mirrors_match_the_headers(c_facts):
    c_prod, c_res = _product(c_facts[0], header_structs)
    assert len(c_prod) == 7 and len(c_res) == 4
    assert struct_mismatches(c_prod, _py_structs(abi, skip=abi.UNCHECKED_STRUCTS)) == []
    assert struct_mismatches(c_res, _py_structs(resident)) == []
    assert [c_prod[n][0] for n in ("SlideEpi", "SlideOp", "SlideGnFin", "SlidePrepCopy", "SlideChainLayer", "SlideHeadArgs",
                                   "SlidePointChainArgs")] == [160, 176, 88, 24, 40, 208, 400]


def test_constants_match_the_headers(c_facts):
    c_prod, c_res = _product(c_facts[1], header_constants)
    assert constant_mismatches(c_prod, _abi_constants()) == []
    assert constant_mismatches(c_res, _resident_constants()) == []
    assert abi.PREC == {"fp32": abi.PREC_F32, "fp16": abi.PREC_F16, "split": abi.PREC_SPLIT}


def test_prototypes_match_the_headers():
    c_protos = {}
    for h in PRODUCT_HEADERS + (RESIDENT_HEADER,):
        c_protos.update(header_prototypes(h))
    assert prototype_mismatches(c_protos, abi.PROTOTYPES) == []
    assert set(header_prototypes(RESIDENT_HEADER)) == abi.EXPERIMENT_FUNCTIONS
    assert _lib.EXPORTS == sorted(set(c_protos) - abi.EXPERIMENT_FUNCTIONS)


def test_libraries_report_the_mirrored_sizes():
    build.build()
    L = _lib.lib()
    assert L.slide_sizeof_epi() == ctypes.sizeof(abi.SlideEpi) and L.slide_sizeof_op() == ctypes.sizeof(abi.SlideOp)
    assert all(getattr(L, n).argtypes == abi.PROTOTYPES[n][1] for n in _lib.EXPORTS)  # the cached handle is the typed one
    if _lib.have_experiments():
        X = resident.lib()
        assert (X.slide_sizeof_rop(), X.slide_sizeof_rstrip(), X.slide_sizeof_rargs()) == tuple(
            ctypes.sizeof(c) for c in (resident.ROp, resident.RStrip, resident.RArgs))
        assert X.slide_sizeof_epi() == ctypes.sizeof(abi.SlideEpi) and X.slide_sizeof_op() == ctypes.sizeof(abi.SlideOp)
        assert X.slide_resident_run.argtypes == abi.PROTOTYPES["slide_resident_run"][1]


def test_the_checker_reports_wrong_mirrors(c_facts):
    """mutated PYTHON copies (never the library): each must be reported"""
    c_prod, _ = _product(c_facts[0], header_structs)
    fields = list(abi.SlideEpi._fields_)
    k = [f[0] for f in fields].index("gs")
    fields[k], fields[k + 1] = fields[k + 1], fields[k]  # two adjacent int32: same size, same total, other order

    class Swapped(ctypes.Structure):
        _fields_ = fields

    good = _py_structs(abi, skip=abi.UNCHECKED_STRUCTS)
    bad = struct_mismatches(c_prod, dict(good, SlideEpi=Swapped))
    assert any("SlideEpi: fields differ" in b for b in bad) and any(b.startswith("SlideEpi.gs:") for b in bad), bad

    class Short(ctypes.Structure):
        _fields_ = list(abi.SlideOp._fields_)[:-1]

    bad = struct_mismatches(c_prod, dict(good, SlideOp=Short))
    assert any(b.startswith("sizeof(SlideOp)") for b in bad) and any("SlideOp: fields differ" in b for b in bad), bad
    assert struct_mismatches(c_prod, {n: c for n, c in good.items() if n != "SlideGnFin"}) == ["struct SlideGnFin is on one side only"]

    c_consts, _ = _product(c_facts[1], header_constants)
    good = _abi_constants()
    assert len(good) == len(c_consts) >= 49
    assert constant_mismatches(c_consts, dict(good, OP_ATTN_TAIL=good["OP_ATTN_TAIL"] + 1)) == ["OP_ATTN_TAIL: C 16, Python 17"]
    assert constant_mismatches(c_consts, dict(good, OP_NEW=40)) == ["constant OP_NEW is on one side only"]
    assert constant_mismatches(c_consts, {n: v for n, v in good.items() if n != "F_OUT_FM"}) == ["constant F_OUT_FM is on one side only"]

    c_protos = {}
    for h in PRODUCT_HEADERS + (RESIDENT_HEADER,):
        c_protos.update(header_prototypes(h))
    r, a = abi.PROTOTYPES["slide_col_sums"]
    assert a[0] is ctypes.c_longlong
    narrow = dict(abi.PROTOTYPES, slide_col_sums=(r, (ctypes.c_int,) + a[1:]))
    assert prototype_mismatches(c_protos, narrow) == ["slide_col_sums: parameter 0 C %s, Python c_int" % ctypes.c_longlong.__name__]
    missing = {n: v for n, v in abi.PROTOTYPES.items() if n != "slide_gather_rows"}
    assert prototype_mismatches(c_protos, missing) == ["function slide_gather_rows is on one side only"]
    r, a = abi.PROTOTYPES["slide_run_ops"]
    assert any("3 parameters in C, 2 in Python" in b for b in prototype_mismatches(c_protos, dict(abi.PROTOTYPES, slide_run_ops=(r, a[:2]))))
    assert any("return type" in b for b in prototype_mismatches(c_protos, dict(abi.PROTOTYPES, slide_hip_version=(ctypes.c_int, ()))))


def _received(name, *values):
    """what a C function with PROTOTYPES[name] receives for `values`: a Python callback of that very prototype echoes its arguments"""
    restype, argtypes = abi.PROTOTYPES[name]
    seen = []
    echo = ctypes.CFUNCTYPE(restype, *argtypes)(lambda *a: seen.append(a) or 0)
    assert echo(*values) == 0
    return seen[0]


def test_typed_handle_passes_full_width():
    """the conversion the typed handle applies, not a library call: a device address or a row count above 2^32 arrives whole
    (without argtypes ctypes passes a Python int as a 32-bit C int)"""
    v = (1 << 40) + 8
    args = abi.PROTOTYPES["slide_gather_rows"][1]
    assert [k for k, a in enumerate(args) if a is ctypes.c_void_p] == [4, 5, 6, 7]
    for k in (4, 5, 6, 7):
        assert ctypes.cast(args[k].from_param(v), ctypes.c_void_p).value == v
    assert _received("slide_gather_rows", 2, 3, 4, 5, v, v + 16, ctypes.c_void_p(v + 32), None) == (2, 3, 4, 5, v, v + 16, v + 32, None)
    rows_t = abi.PROTOTYPES["slide_col_sums"][1][0]
    assert ctypes.sizeof(rows_t) == 8 and "(%d)" % (1 << 33) in repr(rows_t.from_param(1 << 33))
    assert _received("slide_col_sums", 1 << 33, 32, v, v, None, 0) == (1 << 33, 32, v, v, None, None)
    assert abi.ptr(None) is None


def _coord_bwd(L, p, B=1, N=4, np_=4, K=2, C=5, ldg=32, flags=0, null=(), d2=True, dxyz=True, dnew=True):
    a = {n: (None if n in null else p) for n in ("xyz", "new_xyz", "idx", "dout")}
    return L.slide_group_rows_coord_bwd(B, N, np_, K, C, ldg, flags, a["xyz"], a["new_xyz"], a["idx"], p if d2 else None, None, a["dout"],
                                        p if dxyz else None, p if dnew else None, None)


def test_typed_handle_takes_plain_ints_as_pointers():
    """the no-launch calls of tests/test_abi_group_coord.py through _lib.lib(), the pointers as PLAIN PYTHON INTS (what data_ptr()
    returns): same -3 / 0 returns -- every one of them returns before anything is dereferenced or launched"""
    build.build()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert isinstance(p, int)
    for ldg in (0, -32, 24, 48, 1056):
        assert _coord_bwd(L, p, ldg=ldg) == -3, ldg
    assert _coord_bwd(L, p, C=-1) == -3
    assert _coord_bwd(L, p, C=30, flags=0) == -3
    assert _coord_bwd(L, p, C=27, flags=abi.GROUP_ABS) == -3
    assert _coord_bwd(L, p, C=24, flags=abi.GROUP_ABS | abi.GROUP_CENTER) == -3
    assert _coord_bwd(L, p, C=22, flags=abi.GROUP_FP) == -3
    assert _coord_bwd(L, p, C=33, flags=abi.GROUP_NO_XYZ) == -3
    assert _coord_bwd(L, p, K=0) == -3 and _coord_bwd(L, p, K=-2) == -3
    for name in ("xyz", "new_xyz", "idx", "dout"):
        assert _coord_bwd(L, p, null=(name,)) == -3, name
    assert _coord_bwd(L, p, C=5, flags=abi.GROUP_FP, d2=False) == -3
    assert _coord_bwd(L, p, B=0) == 0 and _coord_bwd(L, p, N=0) == 0 and _coord_bwd(L, p, np_=0) == 0 and _coord_bwd(L, p, B=-1) == 0
    assert _coord_bwd(L, p, flags=abi.GROUP_NO_XYZ) == 0
    assert _coord_bwd(L, p, dxyz=False, dnew=False) == 0
    assert _coord_bwd(L, p, flags=abi.GROUP_FP, C=21, dxyz=False, dnew=False) == 0
