"""Static checks on the ambient kernel's generated code (hipcc cross-compiles here, no GPU): one instantiation per
kernel variant plus the one stack walk, names that neither the probe kernels' counts nor the render kernels' tags
pick up, the query kernel's scratch bar in the Cornell instantiation, and an occupancy no lower than the query
kernel's of the same variant in the same compile. Reads the compiler's resource remarks only: names and resource
numbers."""
import re

import pytest

from kernel_isa import RENDER_TAGS, compile_isa, remarks_by_function, variants


@pytest.fixture(scope="module")
def remarks():
    return remarks_by_function(compile_isa()[1])


def _number(block, what):
    return int(re.search(re.escape(what) + r": (\d+)", block).group(1))


def test_one_instantiation_per_variant_and_one_stack_walk(remarks):
    names = [n for n in remarks if "ambient_kernel" in n]
    nvar = len(variants())
    assert nvar == 5 and len(names) == nvar + 1, names
    threaded = [n for n in names if re.search(r"ambient_kernelILj\d+ELi2EE", n)]
    stack = [n for n in names if re.search(r"ambient_kernelILj\d+ELi0EE", n)]
    assert len(threaded) == nvar and len(stack) == 1, names
    assert len(set(re.search(r"ILj(\d+)E", n).group(1) for n in threaded)) == nvar


def test_names_share_no_tag_with_the_other_kernels(remarks):
    """Two template parameters and no trailing bool: the counts by which the tests and tools find the query, occlusion
    and render kernels stay what they were."""
    for n in remarks:
        if "ambient_kernel" in n:
            assert "query_kernel" not in n and "occlusion_kernel" not in n and not any(t in n for t in RENDER_TAGS), n
    for t in RENDER_TAGS[:4]:
        assert len([n for n in remarks if t in n]) == 1, t
    nvar = len(variants())
    assert len([n for n in remarks if "query_kernel" in n]) == nvar + 1
    assert len([n for n in remarks if "occlusion_kernel" in n]) == nvar + 1


def test_cornell_instantiation_meets_the_query_kernel_s_scratch_bar(remarks):
    cornell = [b for n, b in remarks.items() if re.search(r"ambient_kernelILj4ELi2EE", n)]
    assert len(cornell) == 1
    assert _number(cornell[0], "ScratchSize [bytes/lane]") <= 16


def test_occupancy_is_not_below_the_query_kernel_s(remarks):
    """Per variant and walk: the ambient kernel draws a direction and then carries the occlusion kernel's state."""
    amb = {re.search(r"ambient_kernel(ILj\d+ELi\d)EE", n).group(1): b for n, b in remarks.items()
           if "ambient_kernel" in n}
    qry = {re.search(r"query_kernel(ILj\d+ELi\d)EE", n).group(1): b for n, b in remarks.items() if "query_kernel" in n}
    assert set(amb) == set(qry) and len(amb) == len(variants()) + 1
    for k in amb:
        a, q = _number(amb[k], "Occupancy [waves/SIMD]"), _number(qry[k], "Occupancy [waves/SIMD]")
        assert a >= q, (k, a, q)
