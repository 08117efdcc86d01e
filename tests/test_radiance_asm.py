"""Static checks on the radiance kernel's generated code (hipcc cross-compiles here, no GPU): one instantiation per
kernel variant plus the one stack walk, names that neither the probe kernels' counts nor the render kernels' tags
pick up, the query kernel's scratch bar in the Cornell instantiation, and the waves per SIMD that DESIGN.md §6m
records, so that a change that lowers them is seen. Reads the compiler's resource remarks only: names and resource
numbers."""
import re

import pytest

from kernel_isa import RENDER_TAGS, compile_isa, remarks_by_function, variants

# waves per SIMD by (feature word, mode), DESIGN.md §6m's table: mode 2 the threaded program, 0 the stack walk
WAVES = {("4", 2): 8, ("6", 2): 7, ("97", 2): 8, ("815", 2): 5, ("1023", 2): 4, ("1023", 0): 4}


@pytest.fixture(scope="module")
def remarks():
    return remarks_by_function(compile_isa()[1])


def _number(block, what):
    return int(re.search(re.escape(what) + r": (\d+)", block).group(1))


def test_one_instantiation_per_variant_and_one_stack_walk(remarks):
    names = [n for n in remarks if "radiance_kernel" in n]
    nvar = len(variants())
    assert nvar == 5 and len(names) == nvar + 1, names
    threaded = [n for n in names if re.search(r"radiance_kernelILj\d+ELi2EE", n)]
    stack = [n for n in names if re.search(r"radiance_kernelILj\d+ELi0EE", n)]
    assert len(threaded) == nvar and len(stack) == 1, names
    assert len(set(re.search(r"ILj(\d+)E", n).group(1) for n in threaded)) == nvar
    assert len([n for n in remarks if "radiance_sum_kernel" in n]) == 1


def test_names_share_no_tag_with_the_other_kernels(remarks):
    """Two template parameters and no trailing bool: the counts by which the tests and tools find the query, occlusion,
    ambient and render kernels stay what they were."""
    for n in remarks:
        if "radiance_kernel" in n or "radiance_sum_kernel" in n:
            assert not any(k in n for k in ("query_kernel", "occlusion_kernel", "ambient_kernel")), n
            assert not any(t in n for t in RENDER_TAGS), n
    for t in RENDER_TAGS[:4]:
        assert len([n for n in remarks if t in n]) == 1, t
    nvar = len(variants())
    for k in ("query_kernel", "occlusion_kernel", "ambient_kernel"):
        assert len([n for n in remarks if k in n]) == nvar + 1, k
    assert len([n for n in remarks if "render_kernel" in n]) == len([n for n in remarks if re.search(r"\d+render_kernelI", n)])


def test_cornell_instantiation_meets_the_query_kernel_s_scratch_bar(remarks):
    cornell = [b for n, b in remarks.items() if re.search(r"radiance_kernelILj4ELi2EE", n)]
    assert len(cornell) == 1
    assert _number(cornell[0], "ScratchSize [bytes/lane]") <= 16


def test_waves_per_simd_are_what_the_design_records(remarks):
    got = {}
    for n, b in remarks.items():
        m = re.search(r"radiance_kernelILj(\d+)ELi(\d)EE", n)
        if m:
            got[(m.group(1), int(m.group(2)))] = _number(b, "Occupancy [waves/SIMD]")
    assert set(got) == set(WAVES)
    for k, w in WAVES.items():
        assert got[k] >= w, (k, got[k], w)
