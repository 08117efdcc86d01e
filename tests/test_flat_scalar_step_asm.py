"""Static check of what the flat walk's scalar step index bought (render.hip trace_linear with kFlat; DESIGN.md
§4 "Flat walk of small BVHs", "The step index as a scalar"): with no per-lane `next`, no `next == at` test and
no wave-minimum search, the flat kernel's first trace loop (the flat walk; the second is the BVH program's walk
for the uncertified lanes) holds at least 30 static VALU fewer than the 639 it had with them (593), no more
SALU than its 132, and one depth-3 loop fewer (the search loop; the six-face loops of the box-level test and
the quad-run loop remain: 3 of 4). The kernel's resources stay what they were (63 VGPRs, 8 waves per SIMD, no
scratch, 16 SGPR spills), and the kernel it is instantiated from, which walks the BVH program and keeps the
per-lane index, keeps its figures (64 VGPRs, 78 SGPRs, 14 SGPR spills, no scratch). Compiled with
-DRT2_ONLY_VARIANT=0 (the Cornell kernels only)."""
import pytest

from kernel_isa import compile_isa, kernel, loops, resources, salu

FLAT = "ILj1073741828ELi2ELb0E"  # render_kernel<kFeatXform | kFeatFlat, kModeLinear, false>
BVH = "ILj4ELi2ELb0E"  # render_kernel<kFeatXform, kModeLinear, false>
FLAT_TRACE_LOOP_VALU_BEFORE = 639
FLAT_TRACE_LOOP_SALU_BEFORE = 132
FLAT_TRACE_LOOP_INNER_LOOPS_BEFORE = 4


@pytest.fixture(scope="module")
def cornell_isa():
    return compile_isa(("RT2_ONLY_VARIANT=0",))


def _valu(c):
    return sum(v for k, v in c.items() if k.startswith("v_"))


def test_flat_kernel_keeps_its_resources(cornell_isa):
    g = resources(cornell_isa[1], FLAT)
    got = {k: g(k) for k in ("VGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")}
    print("flat kernel:", got)
    assert got["VGPRs"] <= 63 and got["Occupancy [waves/SIMD]"] == 8, got
    assert got["ScratchSize [bytes/lane]"] == 0 and got["VGPRs Spill"] == 0, got
    assert got["SGPRs Spill"] <= 16, got


def test_flat_trace_loop_lost_the_per_lane_index(cornell_isa):
    _, body = kernel(cornell_isa, FLAT)
    lps = loops(body)
    trace = [j for j, (h, d, c) in enumerate(lps) if d == 2 and salu(c) > 60]
    assert len(trace) == 2, [(h, d) for h, d, _ in lps]
    c = lps[trace[0]][2]
    # the first trace loop's own loops: the depth-3 loops listed before the next depth-2 loop
    inner = []
    for h, d, _ in lps[trace[0] + 1:]:
        if d <= 2:
            break
        if d == 3:
            inner.append(h)
    print("flat trace loop: VALU", _valu(c), "SALU", salu(c), "depth-3 loops", inner,
          "| second trace loop: VALU", _valu(lps[trace[1]][2]), "SALU", salu(lps[trace[1]][2]))
    assert salu(c) <= FLAT_TRACE_LOOP_SALU_BEFORE, salu(c)
    assert _valu(c) <= FLAT_TRACE_LOOP_VALU_BEFORE - 30, _valu(c)
    assert len(inner) == FLAT_TRACE_LOOP_INNER_LOOPS_BEFORE - 1, inner


def test_bvh_program_kernel_keeps_its_figures(cornell_isa):
    g = resources(cornell_isa[1], BVH)
    got = {k: g(k) for k in ("VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]")}
    print("BVH-program kernel:", got)
    assert got == {"VGPRs": 64, "TotalSGPRs": 78, "SGPRs Spill": 14, "VGPRs Spill": 0, "ScratchSize [bytes/lane]": 0}, got
