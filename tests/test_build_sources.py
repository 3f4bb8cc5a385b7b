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


def _kernels_under_experiments(text):
    """names of the __global__ functions defined inside an `#ifdef SLIDE_EXPERIMENTS` ... `#endif` region of comment-free source
    text (up to the region's `#else`, if it has one); every #if / #ifdef / #ifndef nests"""
    found, stack = [], []  # one entry per open conditional: "exp" (compiled only with SLIDE_EXPERIMENTS), "product", or "other"
    for line in text.split("\n"):
        d = re.match(r"\s*#\s*(ifdef|ifndef|if|else|elif|endif)\b\s*(\w*)", line)
        if d:
            word, on_exp = d.group(1), d.group(2) == "SLIDE_EXPERIMENTS"
            if word in ("ifdef", "ifndef", "if"):
                stack.append({"ifdef": "exp", "ifndef": "product"}.get(word, "other") if on_exp else "other")
            elif word == "else":  # the #else of `#ifndef SLIDE_EXPERIMENTS` is an experiments region too
                stack[-1] = {"exp": "product", "product": "exp"}.get(stack[-1], "other")
            elif word == "elif":
                stack[-1] = "other"
            else:
                stack.pop()
        elif "exp" in stack and "__global__" in line:
            found.append(line.strip())
    assert not stack
    return found


def test_product_sources_define_no_kernel_under_the_experiments_define():
    """The product library carries only what a default plan dispatches (csrc/launch.h): a kernel that only the experiments build
    compiles lives under csrc/experiments/, not inside an `#ifdef SLIDE_EXPERIMENTS` of a product source, where a reader of the
    file cannot tell what ships.  Guarded DISPATCH (a launch of a template that both builds share) is fine."""
    probe = "#ifdef SLIDE_EXPERIMENTS\n#ifdef SLIDE_TIMELINE\n#endif\n__global__ void k() {}\n#else\n__global__ void p() {}\n#endif\n" \
            "#ifndef SLIDE_EXPERIMENTS\n__global__ void q() {}\n#else\ntemplate <int N> __global__ void r() {}\n#endif\n__global__ void s() {}\n"
    assert _kernels_under_experiments(probe) == ["__global__ void k() {}", "template <int N> __global__ void r() {}"]
    for src, _ in build.SOURCES:
        assert _kernels_under_experiments(_code(os.path.join(build.CSRC, src))) == [], src
