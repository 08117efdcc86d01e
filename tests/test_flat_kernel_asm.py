"""Static checks on the ISA of the kernel that walks flat programs (render.hip kFeatFlat: the Cornell box's
product kernel, the one the benchmark times for scenes with a flat program), in the manner of
test_kernel_asm.py's checks of the kernel it is instantiated from: 8 waves per SIMD within 64 VGPRs, no
scratch, and the quad-run loops of both of its traces (the flat walk and the BVH program's walk for the
uncertified lanes) keep the scalar-issue code generation."""
import re
import subprocess

import pytest

from kernel_isa import HIPCC, SRC, compile_isa, kernel, loops, makefile_hipflags, resources, salu

FLAT = "ILj1073741828ELi2ELb0E"  # render_kernel<kFeatXform | kFeatFlat, kModeLinear, false>


@pytest.fixture(scope="module")
def isa():
    return compile_isa()


def test_flat_kernel_keeps_8_waves_without_scratch(isa):
    g = resources(isa[1], FLAT)
    assert g("VGPRs") <= 64 and g("Occupancy [waves/SIMD]") == 8
    assert g("VGPRs Spill") == 0 and g("ScratchSize [bytes/lane]") == 0
    scratch, body = kernel(isa, FLAT)
    assert scratch == 0 and not re.search(r"scratch_store|scratch_load|buffer_store.*Spill", body)


def test_flat_kernel_quad_run_loops_keep_the_scalar_issue_code_generation(isa):
    """Two traces, so two quad-run loops (depth 3, a scalar record load, v_or3 rejection words): each holds three
    separate QUADAA interior tests (6 v_or3), no exec-mask save per quad and at most 28 SALU; and the kernel
    trace loops stay near the 140 SALU of the kernel they come from (the flat walk 156 with its entry rule, the
    second trace 146; test_kernel_asm.py allows that kernel 150 for its 140, the same headroom here)."""
    _, body = kernel(isa, FLAT)
    lps = loops(body)
    quad = [c for h, d, c in lps if d == 3 and c["v_or3_b32"] > 0 and any(k.startswith("s_load") for k in c)]
    assert len(quad) == 2, [(h, d) for h, d, _ in lps]
    for c in quad:
        assert c["v_or3_b32"] == 6, ("per-axis QUADAA bodies merged", c["v_or3_b32"])
        assert c["s_and_saveexec_b64"] == 0, c["s_and_saveexec_b64"]
        assert salu(c) <= 28, salu(c)
    trace = [c for h, d, c in lps if d == 2 and salu(c) > 60]
    assert len(trace) == 2 and all(salu(c) <= 170 for c in trace), [salu(c) for c in trace]


def test_certificate_probe_build_compiles(tmp_path):
    """RT2_EXP_TWICE bit 16384 probes the flat walk's certificate rule (render.hip); with every probe bit set the
    Cornell build (RT2_ONLY_VARIANT=0: the flat kernel and the kernel it comes from) still compiles."""
    r = subprocess.run([HIPCC, *makefile_hipflags(), "--cuda-device-only", "-c", "-o",
                        str(tmp_path / "k0.o"), "-DRT2_ONLY_VARIANT=0", "-DRT2_EXP_TWICE=32767", SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
