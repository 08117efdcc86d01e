"""Static check that evaluating the flat walk's certificate once per trace (render.hip trace_linear with kFlat;
DESIGN.md §4 "Flat walk of small BVHs") took scalar work out of the flat kernel and put none in: the two lane
masks the entry rule's verdict was carried in are gone, so the kernel reports no more SGPR spills than the 20 it
had with them, and its first trace loop (the flat walk; the second is the BVH program's walk for the uncertified
lanes) holds no more static SALU than the 156 it had with the entry rule in it. Compiled with
-DRT2_ONLY_VARIANT=0 (the Cornell kernels only: the flat kernel and the kernel it is instantiated from)."""
import pytest

from kernel_isa import compile_isa, kernel, loops, resources, salu

FLAT = "ILj1073741828ELi2ELb0E"  # render_kernel<kFeatXform | kFeatFlat, kModeLinear, false>
SGPR_SPILLS_BEFORE = 20
FLAT_TRACE_LOOP_SALU_BEFORE = 156


@pytest.fixture(scope="module")
def cornell_isa():
    return compile_isa(("RT2_ONLY_VARIANT=0",))


def test_flat_kernel_spills_no_more_sgprs(cornell_isa):
    spills = resources(cornell_isa[1], FLAT)("SGPRs Spill")
    print("flat kernel SGPR spills:", spills)
    assert spills <= SGPR_SPILLS_BEFORE


def test_flat_trace_loop_holds_no_more_salu(cornell_isa):
    _, body = kernel(cornell_isa, FLAT)
    trace = [salu(c) for h, d, c in loops(body) if d == 2 and salu(c) > 60]
    print("flat kernel trace loops' SALU:", trace)
    assert len(trace) == 2, trace
    assert trace[0] <= FLAT_TRACE_LOOP_SALU_BEFORE, trace
