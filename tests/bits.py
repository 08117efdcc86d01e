"""What the tests that compare results bit for bit share: a float32 array's words, the comparison, and the call
that must be refused."""
import numpy as np
import pytest


def f32_bits(x):
    """The uint32 words of x as float32 (converted if it is anything else)."""
    return np.asarray(x, np.float32, order="C").view(np.uint32)


def same_bits(a, b):
    """The same shape and the same 32-bit words. Two arrays of one 4-byte type (float32, int32, uint32) are compared as
    they lie in memory; anything else (a float64 result of a numpy statement, a list, two types) is first converted
    to float32, both sides."""
    a, b = np.asarray(a, order="C"), np.asarray(b, order="C")
    if a.dtype == b.dtype and a.dtype.itemsize == 4:
        a, b = a.view(np.uint32), b.view(np.uint32)
    else:
        a, b = f32_bits(a), f32_bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def refused(call):
    """call() must raise Rt2Error with code -1 (RT2_ERR_INVALID); returns the exception."""
    from raytrace2_amd import Rt2Error
    with pytest.raises(Rt2Error) as e:
        call()
    assert e.value.code == -1
    return e.value
