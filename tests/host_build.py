"""The stand-alone host programs of tests/cpp built with g++ for the CPU tests, once per process, source and flag
set, and run: the named flag sets each program is built with, the product's host sources compiled to objects once
per flag set and linked into every program that needs them, the runner of the sanitized programs and the reader of
their `name k=v k=v` lines. Sanitizers are for these programs alone (each has its own main); nothing here loads one
into python."""
import atexit
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytrace2_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

# the flag sets, each as its programs have always been built
_HIP = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC]  # scene.h includes the HIP vector types
COMPILER = ["-O1", "-std=c++17", "-ffp-contract=off", *_HIP]  # the harnesses that link the product's compiler
COMPILER_O2 = ["-O2", "-std=c++17", "-ffp-contract=off", *_HIP]  # box_cert, compile_digest
PAIRS = ["-O1", "-std=c++17", *_HIP]  # program_pairs (no float arithmetic of its own)
HOST = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC]  # filter / query hosts
PLAN = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]  # launch_plan_host
MIRROR = ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]  # the mirror_*.cpp users of the C++ header
SAN = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]  # with COMPILER
HOST_SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]  # with HOST and PLAN
SANITIZE = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer",  # test_sanitize.py
            "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-pthread", *_HIP]
# the product's loader and scene compiler; image.cpp and oracle/rt_oracle.cpp are linked by name as well
COMPILER_SOURCES = ("json.cpp", "scene.cpp", "compile.cpp")
_LIB = os.path.join(ROOT, "raytrace2_amd", "lib")
LIBRT2 = ["-L", _LIB, "-lrt2", "-Wl,-rpath," + _LIB]  # the built library, for the mirrors that link

SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
SANITIZE_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:halt_on_error=1",
                "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}  # test_sanitize.py
_serial = itertools.count()  # one file name per build


@functools.lru_cache(maxsize=None)
def _outdir():
    d = tempfile.mkdtemp(prefix="rt2_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _gxx(args):
    r = subprocess.run(["g++", *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@functools.lru_cache(maxsize=None)
def _object(source, flags):
    """A product source (a name in csrc, or a path from the root) compiled under `flags`, once."""
    src = os.path.join(ROOT, source) if "/" in source else os.path.join(CSRC, source)
    obj = os.path.join(_outdir(), f"{os.path.basename(source)}.{next(_serial)}.o")
    _gxx([*flags, "-c", "-o", obj, src])
    return obj


@functools.lru_cache(maxsize=None)
def _program(source, flags, product, link):
    exe = os.path.join(_outdir(), f"{source[:-4]}.{next(_serial)}")
    _gxx([*flags, "-o", exe, os.path.join(CPP, source), *[_object(p, flags) for p in product], *link])
    return exe


def program(source, flags, product=(), defines=(), link=()):
    """The path of tests/cpp/<source> built under `flags` and -D<define> for each of `defines`, with the product
    sources `product` (compiled under the same flags and defines) and the link arguments `link`."""
    return _program(source, (*flags, *["-D" + d for d in defines]), tuple(product), tuple(link))


def syntax_only(source):
    """tests/cpp/<source> must compile against include/rt2/RayTracer.hpp (nothing is linked)."""
    _gxx([*MIRROR, "-fsyntax-only", os.path.join(CPP, source)])


def run(exe, args, timeout, env=SAN_ENV, drop=()):
    """stdout of a program that must end with status 0 and no sanitizer report, under `env` on top of the
    environment less the variables `drop`."""
    e = dict(os.environ, **env)
    for k in drop:
        e.pop(k, None)
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=e, timeout=timeout)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    return r.stdout


def parse(stdout, name=lambda s: s):
    """{name: {k: int(v)}} of a program's `name k=v k=v` lines."""
    got = {}
    for line in stdout.splitlines():
        f = line.split()
        got[name(f[0])] = {k: int(v) for k, v in (x.split("=") for x in f[1:])}
    return got
