"""The numpy statement of raytrace2_amd/csrc/present.h (PresentPixel): a float32 colour image to RGBA8, the
arithmetic of Pixels(), and the edge-value image the host and the GPU tests share."""
import numpy as np

F32 = np.float32

# -0, 0, the smallest float above 0, the largest below 1, 1, 1 + ulp, 1e30, +inf, -inf, NaN
EDGE_VALUES = np.array([-0.0, 0.0, np.nextafter(F32(0), F32(1)), np.nextafter(F32(1), F32(0)), 1.0,
                        np.nextafter(F32(1), F32(2)), 1e30, np.inf, -np.inf, np.nan], F32)
# the byte present.h defines for each of them
EDGE_BYTES = np.array([0, 0, 0, 255, 255, 255, 255, 255, 0, 0], np.uint8)


def present(color):
    """(..., 3) float32 -> (..., 4) uint8: per channel v = c > 0 ? c : 0; v = v < 1 ? v : 1;
    byte = floor((double)v * 255.999); alpha 255. Comparisons with NaN are false."""
    c = np.ascontiguousarray(color, F32)
    assert c.shape[-1] == 3
    with np.errstate(invalid="ignore"):
        v = np.where(c > F32(0), c, F32(0)).astype(F32)
        v = np.where(v < F32(1), v, F32(1)).astype(F32)
    b = np.floor(v.astype(np.float64) * 255.999).astype(np.uint8)
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = b
    return out


def edge_cases():
    """(3, 10, 3) float32: pixel (k, e) holds edge value e in channel k and random values in the other two."""
    rng = np.random.default_rng(7)
    c = (rng.random((3, len(EDGE_VALUES), 3), F32) * F32(2) - F32(0.5)).astype(F32)
    for k in range(3):
        c[k, :, k] = EDGE_VALUES
    return c


def edge_image(w, h, seed=11):
    """(h, w, 3) float32: random values in [-0.5, 1.5]; an image of 210 pixels or more (33 x 9 is one) also holds every
    edge value in every channel, each at a pixel of its own, seven pixels apart."""
    rng = np.random.default_rng(seed)
    c = (rng.random((h, w, 3), F32) * F32(2) - F32(0.5)).astype(F32)
    flat = c.reshape(-1, 3)
    if flat.shape[0] >= 3 * len(EDGE_VALUES) * 7:
        j = 0
        for k in range(3):
            for e in EDGE_VALUES:
                flat[j * 7 + 3, k] = e
                j += 1
    return c
