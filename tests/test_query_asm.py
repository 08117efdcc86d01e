"""Static checks on the query kernel's generated code (hipcc cross-compiles here, no GPU): one instantiation per
kernel variant plus the one stack walk, names that none of the render kernels' tags pick up, and no scratch in the
Cornell instantiation. Reads the compiler's resource remarks only."""
import re

import pytest

from kernel_isa import RENDER_TAGS, compile_isa, remarks_by_function, variants


@pytest.fixture(scope="module")
def remarks():
    return remarks_by_function(compile_isa()[1])


def test_one_instantiation_per_variant_and_one_stack_walk(remarks):
    names = [n for n in remarks if "query_kernel" in n]
    nvar = len(variants())
    assert nvar == 5 and len(names) == nvar + 1, names
    threaded = [n for n in names if re.search(r"query_kernelILj\d+ELi2EE", n)]
    stack = [n for n in names if re.search(r"query_kernelILj\d+ELi0EE", n)]
    assert len(threaded) == nvar and len(stack) == 1, names
    assert len(set(re.search(r"ILj(\d+)E", n).group(1) for n in threaded)) == nvar


def test_names_share_no_tag_with_the_render_kernels(remarks):
    for n in remarks:
        if "query_kernel" in n:
            assert not any(t in n for t in RENDER_TAGS), n
    # and the render kernels' tags still find exactly one kernel each
    for t in RENDER_TAGS[:4]:
        assert len([n for n in remarks if t in n]) == 1, t


def test_cornell_instantiation_has_no_more_scratch_than_the_bench_kernels(remarks):
    cornell = [b for n, b in remarks.items() if re.search(r"query_kernelILj4ELi2EE", n)]
    assert len(cornell) == 1
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", cornell[0]).group(1))
    assert scratch <= 16, scratch
