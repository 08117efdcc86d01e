"""Static check that evaluating the flat walk's certificate once per trace (render.hip trace_linear with kFlat;
DESIGN.md §4 "Flat walk of small BVHs") took scalar work out of the flat kernel and put none in: the two lane
masks the entry rule's verdict was carried in are gone, so the kernel reports no more SGPR spills than the 20 it
had with them, and its first trace loop (the flat walk; the second is the BVH program's walk for the uncertified
lanes) holds no more static SALU than the 156 it had with the entry rule in it. Compiled with
-DRT2_ONLY_VARIANT=0 (the Cornell kernels only: the flat kernel and the kernel it is instantiated from)."""
import re
import subprocess

import pytest

from test_kernel_asm import SRC, _kernel, _loops, _salu, makefile_hipflags

FLAT = "ILj1073741828ELi2ELb0E"  # render_kernel<kFeatXform | kFeatFlat, kModeLinear, false>
SGPR_SPILLS_BEFORE = 20
FLAT_TRACE_LOOP_SALU_BEFORE = 156


@pytest.fixture(scope="module")
def cornell_isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_cert_once") / "render0.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", *makefile_hipflags(), "--cuda-device-only", "-S", "-o", str(out),
                        "-DRT2_ONLY_VARIANT=0", SRC, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text(), r.stderr


def test_flat_kernel_spills_no_more_sgprs(cornell_isa):
    _, remarks = cornell_isa
    blk = [b for b in re.split(r"remark: Function Name: ", remarks)[1:] if FLAT in b.split()[0]]
    assert len(blk) == 1
    spills = int(re.search(r"SGPRs Spill: (\d+)", blk[0]).group(1))
    print("flat kernel SGPR spills:", spills)
    assert spills <= SGPR_SPILLS_BEFORE, blk[0]


def test_flat_trace_loop_holds_no_more_salu(cornell_isa):
    _, body = _kernel(cornell_isa, FLAT)
    trace = [_salu(c) for h, d, c in _loops(body) if d == 2 and _salu(c) > 60]
    print("flat kernel trace loops' SALU:", trace)
    assert len(trace) == 2, trace
    assert trace[0] <= FLAT_TRACE_LOOP_SALU_BEFORE, trace
