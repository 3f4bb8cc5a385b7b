"""CPU: slide_amd/build.py's source lists against the files under slide_amd/csrc, and csrc/launch.h against the definitions.

The libraries are shared objects: a .hip nobody lists, or a launch entry point nobody defines, would otherwise show only when the
library is loaded.  The lists and the directory are compared in both directions, and every function that launch.h declares must
be defined at file scope in exactly one .hip.  Text only; no device and no compiler is needed."""
import glob
import os
import re

from slide_amd import build


def _hip_files(sub=""):
    return {os.path.join(sub, os.path.basename(p)) for p in glob.glob(os.path.join(build.CSRC, sub, "*.hip"))}


def _code(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def test_sources_match_the_directory():
    product = [s for s, _ in build.SOURCES]
    assert len(set(product)) == len(product)
    assert set(product) == _hip_files()
    exp = [s for s, _ in build.SOURCES_EXP]
    assert len(set(exp)) == len(exp)
    assert set(product) <= set(exp)  # the experiments library is the product sources plus the opt-in variants
    assert set(exp) - set(product) == _hip_files("experiments")


def test_launch_header_functions_are_defined_once():
    declared = re.findall(r"^int\s+(slide_launch_\w+)\s*\([^;{]*\)\s*;", _code(os.path.join(build.CSRC, "launch.h")), flags=re.M)
    assert len(set(declared)) == len(declared)
    assert {"slide_launch_gemm", "slide_launch_rows_op", "slide_launch_gemm_xs"} <= set(declared)  # (the scan sees all three forms)
    code = {s: _code(os.path.join(build.CSRC, s)) for s, _ in build.SOURCES_EXP}
    for name in declared:
        # a definition at file scope: `int name(...) {` starting in column 0 (a call or a declaration does not match)
        definition = re.compile(r"^int\s+%s\s*\([^;{]*\)\s*\{" % name, flags=re.M)
        where = [s for s, text in code.items() if definition.search(text)]
        assert len(where) == 1, "%s is defined in %s" % (name, where or "no source")
    # and nothing named slide_launch_* is defined without a declaration in the header
    defined = set()
    for text in code.values():
        defined |= set(re.findall(r"^int\s+(slide_launch_\w+)\s*\([^;{]*\)\s*\{", text, flags=re.M))
    assert defined == set(declared)
