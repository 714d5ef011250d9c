"""CPU test: libdsa_hip.so builds for gfx950, loads, and exports every symbol include/dsa.h declares
(no compute call is made — there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_in_header():
    txt = open(os.path.join(ROOT, "include", "dsa.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dsa_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_header_symbols(dsa):
    csrc = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-j4", "libdsa_hip.so"])
    lib = ctypes.CDLL(os.path.join(csrc, "libdsa_hip.so"))
    names = declared_in_header()
    assert len(names) >= 45
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # the ctypes binding declares the same set
    bound = {"dsa_" + n for n in dsa.Binding.declared_symbols()}
    assert bound == set(names), sorted(bound ^ set(names))


def test_header_is_plain_c(tmp_path):
    """include/dsa.h is the drop-in boundary: it must be consumable from C (cgo / ccall / ctypes generators) as well as C++."""
    src = tmp_path / "use_header.c"
    src.write_text('#include "dsa.h"\nint main(void) { dsa_vec_t* v = 0; (void)v; return DSA_OK; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + inc, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, "-x", "c++", str(src)])


def test_product_code_object_is_gfx950_only():
    csrc = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc")
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o",
                          "--input=" + os.path.join(csrc, "libdsa_hip.so")], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        targets = [t for t in out.stdout.split() if "amdgcn" in t]
        assert targets and all("gfx950" in t for t in targets), targets


def test_product_carries_no_library_sort():
    """Every sort and scan of the bulk builder is hand-written for gfx950 (csrc/build.hip: LSD radix passes, flag scans) — also on the
    general path for composites wider than 64 bits, which called rocPRIM until round 3: no rocprim symbol in the shared library."""
    so = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so")
    out = subprocess.run(["nm", "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "rocprim" not in out
    # (the device code objects are embedded in the same file: their kernel names would show up in .hip_fatbin strings)
    raw = open(so, "rb").read()
    assert b"rocprim" not in raw


def test_product_does_not_reference_the_oracle():
    """The product path must not import, link or execute anything under oracle/."""
    pkg = os.path.join(ROOT, "dynamicsparsearrays.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".jl")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "liboracle" not in txt and "oracle.hpp" not in txt and "ora_" not in txt.replace("ora_`", ""), (dirpath, f)



def test_shard_range_matches_the_host_layer(dsa):
    """dsa_shard_range (pure host arithmetic, callable without a GPU) and sharding.column_range split n columns the same way;
    the ranges tile 1..n without gaps or overlaps."""
    import ctypes as C
    from dsa_amd import sharding
    b = dsa.product()
    for n, G in [(10, 1), (10, 3), (1_000_000, 8), (7, 8), (0, 2), (10_000_000, 8)]:
        end = 0
        for g in range(G):
            c0, nc = C.c_int64(), C.c_int64()
            b.call("shard_range", n, G, g, C.byref(c0), C.byref(nc))
            assert (c0.value, nc.value) == sharding.column_range(g, G, n)
            assert c0.value == end
            end += nc.value
        assert end == n
    c0, nc = C.c_int64(), C.c_int64()
    import pytest
    with pytest.raises(dsa.DsaArgumentError):
        b.call("shard_range", 10, 2, 2, C.byref(c0), C.byref(nc))


def test_missing_rccl_is_a_status_code_not_a_crash():
    """A box without RCCL: dsa_comm_unique_id / dsa_comm_init must come back with DSA_ERCCL and a message (the loader once built that
    message from two dlerror() calls — the second returns NULL — and took the host process down with it).  DSA_RCCL_LIB names the only
    library that is tried; run in a child process because the loader binds once per process.  No GPU call is made."""
    code = r"""
import ctypes as C, os, sys
lib = C.CDLL(os.path.join(sys.argv[1], "dynamicsparsearrays.jl_amd", "csrc", "libdsa_hip.so"))
lib.dsa_last_error_message.restype = C.c_char_p
buf = (C.c_uint8 * 128)()
rc = lib.dsa_comm_unique_id(buf)
msg = lib.dsa_last_error_message().decode()
assert rc == 10, rc                       # DSA_ERCCL
assert "librccl.so not found" in msg, msg
out = C.c_void_p()
rc = lib.dsa_comm_init(0, 2, buf, C.byref(out))
assert rc in (10, 7), rc                  # DSA_ERCCL (DSA_EHIP without any device: the current-device query comes first)
print("ok")
"""
    env = dict(os.environ, DSA_RCCL_LIB="/nonexistent/librccl.so")
    r = subprocess.run([os.sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_julia_wrapper_binds_only_declared_symbols():
    """The Julia wrapper cannot be executed here (no Julia toolchain): at least every symbol it `ccall`s must be declared in
    include/dsa.h, and the argument count of each ccall must match the C prototype."""
    jl = open(os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia", "DynamicSparseArraysAMD.jl")).read()
    hdr = open(os.path.join(ROOT, "include", "dsa.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    def c_class(a):
        a = a.strip()
        if "*" in a or "[" in a:
            return "ptr"
        for t, k in (("int64_t", "i64"), ("int32_t", "i32"), ("double", "f64")):
            if re.search(r"\b" + t + r"\b", a):
                return k
        raise AssertionError(a)

    def jl_class(a):
        a = a.strip()
        if a.startswith(("Ptr{", "Ref{")):
            return "ptr"
        return {"Int64": "i64", "Int32": "i32", "Float64": "f64", "Cdouble": "f64"}[a]

    protos = {}
    for m in re.finditer(r"\b(dsa_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = [] if args in ("", "void") else [c_class(a) for a in args.split(",") if a.strip()]
    used = re.findall(r"ccall\(\(:(dsa_[a-z0-9_]+),\s*libdsa\),\s*\w+,\s*\(((?:[^()]|\([^()]*\))*)\)", jl)
    assert len(used) >= 30
    for name, argt in used:
        assert name in protos, name
        got = [jl_class(a) for a in re.split(r",\s*(?![^{}]*\})", argt) if a.strip()]
        assert got == protos[name], (name, got, protos[name])
    # entry points stamped out with @eval: the symbol list of the `for` and the argument tuple of the ccall inside it
    stamped = re.findall(r"for \(fname, sym\) in \(([^\n]*)\)\n(.*?)\nend\n", jl, flags=re.S)
    assert len(stamped) == 2
    for syms, body in stamped:
        argt = re.search(r"ccall\(\(\$\(QuoteNode\(sym\)\), libdsa\), Int32,\s*\(((?:[^()]|\([^()]*\))*)\)", body).group(1)
        got = [jl_class(a) for a in re.split(r",\s*(?![^{}]*\})", argt) if a.strip()]
        for name in re.findall(r":(dsa_[a-z0-9_]+)", syms):
            assert got == protos[name], (name, got, protos[name])
    assert "ccall((sym" not in jl          # ccall needs a literal (symbol, library) pair
    # symbols passed indirectly (the view / slice helpers take the symbol as an argument)
    for name in re.findall(r":(dsa_[a-z0-9_]+)", jl):
        assert name in protos, name


# the twelve names the reference exports (reference src/DynamicSparseArrays.jl:5-16)
REFERENCE_EXPORTS = ["DynamicSparseVector", "DynamicSparseMatrix", "DynamicMatrixColView", "dynamicsparsevec", "dynamicsparse",
                     "nbpartitions", "deletepartition!", "deletecolumn!", "deleterow!", "addrow!", "closefillmode!", "shrink_size!"]


def _exports(src):
    names = []
    for m in re.finditer(r"^export\s+((?:[^\n]*,\s*\n)*[^\n]*)", src, flags=re.M):
        names += [n.strip() for n in m.group(1).replace("\n", " ").split(",") if n.strip()]
    return names


def test_julia_modules_export_the_reference_surface():
    """Drop-in surface: the wrapper module AND the module offered under the reference's own name export every name the
    reference exports; the latter exports nothing else.  Every exported name is defined in the wrapper; the key-mapping
    layer (keyint / keyfrom, generic K and L) and the arbitrary-combine pre-fold are present."""
    jdir = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "julia")
    amd = open(os.path.join(jdir, "DynamicSparseArraysAMD.jl")).read()
    dropin = open(os.path.join(jdir, "DynamicSparseArrays.jl")).read()
    assert re.search(r"^module DynamicSparseArrays\s*$", dropin, flags=re.M)
    assert 'include("DynamicSparseArraysAMD.jl")' in dropin and "using .DynamicSparseArraysAMD" in dropin
    assert sorted(_exports(dropin)) == sorted(REFERENCE_EXPORTS)
    amd_exports = _exports(amd)
    for name in REFERENCE_EXPORTS:
        assert name in amd_exports, name
        base = re.escape(name)
        assert re.search(r"(?:function\s+|struct\s+|^)" + base + r"(?:\{[^}]*\})?\s*[\(\{<\s]", amd, flags=re.M), name
    for needed in ("keyint(k::Integer)", "keyint(k::Char)", "keyfrom(::Type{Char}", "struct KeyMap{K}", "function _prefold",
                   "Base.iterate(dv::DynamicMatrixColView", "mutable struct DynamicSparseMatrix{K,L}", "mutable struct DynamicSparseVector{K}"):
        assert needed in amd, needed
    # an unsupported combine is never silently mapped to +
    assert "get(COMBINE, combine, Int32(0))" not in amd


def test_development_switches_are_one_table_and_off_by_default(dsa):
    """Release configuration (include/dsa.h: dsa_dev_switches).  Every DSA_* environment variable the library reads is either one of
    the four documented configuration variables or a development switch listed in the ONE table of csrc/dsa_host.hip, and those are
    read through dev_env(), which returns nothing unless DSA_DEV=1: no plain getenv of a switch is left in the sources.  No GPU call."""
    csrc = os.path.join(ROOT, "dynamicsparsearrays.jl_amd", "csrc")
    names, enabled = dsa.dev_switches(dsa.product())
    assert enabled == (os.environ.get("DSA_DEV") == "1")
    assert "DSA_TIGHT" in names and "DSA_PARBATCH" in names and len(names) == len(set(names))
    config = {"DSA_POOL_MAX_MB", "DSA_RCCL_LIB", "DSA_WAIT_POLICY", "DSA_ROCTX", "DSA_DEV"}
    used_dev, used_plain = set(), set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            txt = open(os.path.join(csrc, f)).read()
            used_dev |= set(re.findall(r'dev_env\("([A-Z0-9_]+)"\)', txt))
            used_plain |= set(re.findall(r'(?<![a-z_])getenv\("([A-Z0-9_]+)"\)', txt))
    assert used_plain <= config, used_plain - config
    assert used_dev == set(names), used_dev ^ set(names)
    assert not (set(names) & config)
    # a child process without DSA_DEV reports the switches as ignored, one with DSA_DEV=1 as honoured
    code = ("import sys; sys.path.insert(0, %r); import dsa_loader; d = dsa_loader.load(); print(d.dev_switches(d.product())[1])" % ROOT)
    for dev, want in ((None, "False"), ("1", "True"), ("0", "False")):
        env = {k: v for k, v in os.environ.items() if k != "DSA_DEV"}
        env["DSA_TIGHT"] = "0"
        if dev is not None:
            env["DSA_DEV"] = dev
        r = subprocess.run([os.sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith(want), (dev, r.stdout, r.stderr)
