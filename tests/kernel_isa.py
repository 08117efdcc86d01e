"""render.hip compiled to gfx950 ISA for the static tests (hipcc cross-compiles here, no GPU), once per process and
set of defines, and what those tests read out of it: the compiler's resource remarks per function, a kernel's
body by its tag, a body's loops and their opcode counts."""
import atexit
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

from conftest import ROOT

SRC = os.path.join(ROOT, "raytrace2_amd", "csrc", "render.hip")
HIPCC = "/opt/rocm/bin/hipcc"
# the tags by which the tests and the tools find render kernels in the ISA
RENDER_TAGS = ["ILj4ELi2ELb0E", "ILj6ELi2ELb0E", "ILj815ELi2ELb0E", "ILj1073741828ELi2ELb0E", "render_kernel",
               "features_kernel"]


def makefile_hipflags():
    """The kernel's compile flags as the build uses them (raytrace2_amd/csrc/Makefile HIPFLAGS)."""
    mk = open(os.path.join(ROOT, "raytrace2_amd", "csrc", "Makefile")).read()
    line = re.search(r"^HIPFLAGS\s*:=(.*)$", mk, re.M).group(1)
    return [f for f in line.split() if not f.startswith("$(") and f not in ("-fPIC", "-Wall")]


def variants():
    """The entries of render.hip kVariants."""
    src = open(SRC).read()
    body = re.search(r"constexpr uint32_t kVariants\[\] = \{(.*?)\n\};", src, re.S).group(1)
    return [l for l in body.split("\n") if l.strip().startswith("kFeat")]


@functools.lru_cache(maxsize=None)
def _outdir():
    d = tempfile.mkdtemp(prefix="rt2_isa_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def compile_isa(defines=()):
    """(asm text, resource remarks) of render.hip's device code under the Makefile's flags and -D<define> for each of
    `defines` (a tuple)."""
    flags = makefile_hipflags()
    assert "--offload-arch=gfx950" in flags
    out = os.path.join(_outdir(), "render_" + "_".join(defines).replace("=", "-") + ".s")
    r = subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", "-o", out, *["-D" + d for d in defines], SRC,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read(), r.stderr


def remarks_by_function(remarks):
    """The remarks' block of each function, by its mangled name."""
    return {b.split()[0]: b for b in re.split(r"remark: Function Name: ", remarks)[1:]}


def resources(remarks, tag):
    """Reader of the resource numbers of the one function whose name holds `tag`: g("VGPRs"), ..."""
    blk = [b for n, b in remarks_by_function(remarks).items() if tag in n]
    assert len(blk) == 1, tag
    return lambda k: int(re.search(re.escape(k) + r": (\d+)", blk[0]).group(1))


def kernel(isa, tag):
    """(scratch bytes per lane, body) of the one kernel whose name holds `tag`; isa: compile_isa()'s pair."""
    s, remarks = isa
    name = [n for n in remarks_by_function(remarks) if tag in n]
    assert len(name) == 1, tag
    body = s.split(f"\n{name[0]}:", 1)[1].split(".Lfunc_end", 1)[0]
    return resources(remarks, tag)("ScratchSize [bytes/lane]"), body


def loops(body, lines=False):
    """Every loop of a kernel body: (header label, depth, opcode counts of the loop's blocks), and with
    lines=True the loop's instruction lines as a fourth element."""
    blocks, cur = [], None
    for line in body.split("\n"):
        if line.startswith(".LBB") or line.startswith("; %bb"):
            cur = [line.split()[0].rstrip(":") if line.startswith(".LBB") else line.split()[1], [line], [], []]
            blocks.append(cur)
        elif cur is not None and line.strip().startswith(";"):
            if not cur[2]:
                cur[1].append(line)
        elif cur is not None and line.startswith("\t") and not line.strip().startswith("."):
            cur[2].append(line.split()[0])
            cur[3].append(line.strip())
    out = []
    for b in blocks:
        m = re.search(r"Loop Header: Depth=(\d+)", " ".join(b[1]))
        if not m:
            continue
        h = b[0].lstrip(".L")
        c = collections.Counter()
        ls = []
        for bb in blocks:
            txt = " ".join(bb[1])
            if bb is b or f"Header={h} " in txt or f"Parent Loop {h} " in txt or txt.endswith(f"Header={h}"):
                c.update(bb[2])
                ls.extend(bb[3])
        out.append((b[0], int(m.group(1)), c, ls) if lines else (b[0], int(m.group(1)), c))
    return out


def salu(c):
    return sum(v for k, v in c.items()
               if k.startswith("s_") and not k.startswith(("s_load", "s_waitcnt", "s_nop", "s_cbranch", "s_branch")))
