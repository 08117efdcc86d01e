"""Multi-GPU plumbing for callers that move the band stacks themselves: the interleaved row-band
partition of the framebuffer and a torch.distributed gather of every rank's bands to rank 0 (RCCL
over xGMI with device tensors on MI355X, gloo with host tensors in the CPU tests). The product's own
gather is rt2_tracer_gather in librt2.so (ncclGather + the root's de-interleave kernel); this module
is the same layout in torch terms.

The render itself needs no communication: pixels are independent (RayTracer.cpp:62-69) and the
sample streams are keyed by (seed, global pixel, frame), so the gathered image is bit-identical to
a single-GPU render. The only exchange is this gather.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist

from ._native import check, lib
from .tracer import _fp, local_rows


def band_rows_max(height: int, band_h: int, world: int) -> int:
    """Rows every rank sends (its band stack padded to the largest rank's; rt2_band_rows_max, the
    same function the C ABI's gather uses)."""
    return check(lib.rt2_band_rows_max(int(height), int(band_h), int(world)))


def deinterleave(stacks: np.ndarray, height: int, band_h: int) -> np.ndarray:
    """Rank-major padded band stacks (world, max_rows, W, C) -> the image (H, W, C), through the C
    ABI's host de-interleave (rt2_layout.h BandSource, the map of the root's GPU kernel)."""
    stacks = np.ascontiguousarray(stacks, np.float32)
    world, max_rows, w, c = stacks.shape
    out = np.empty((height, w, c), np.float32)
    check(lib.rt2_deinterleave_host(_fp(stacks), _fp(out), w, height, int(band_h), world, max_rows, c))
    return out


def deinterleave_estimate(stacks: np.ndarray, stacks2: np.ndarray, height: int, band_h: int, frames: int):
    """Rank-major padded band stacks (world, max_rows, W, 3) of the sums and of the sums of squares over `frames`
    frames -> (sums, means, variance of the mean) in image order, (H, W, 3), (H, W, 3) and (H, W): the host
    statement of gather_estimate()'s kernel (rt2_deinterleave_estimate_host), for stacks gathered by other means."""
    stacks = np.ascontiguousarray(stacks, np.float32)
    stacks2 = np.ascontiguousarray(stacks2, np.float32)
    world, max_rows, w, c = stacks.shape
    if c != 3 or stacks2.shape != stacks.shape or max_rows != band_rows_max(height, band_h, world):
        raise ValueError("deinterleave_estimate: need two (world, band_rows_max, W, 3) stacks")
    image, mean = np.empty((height, w, 3), np.float32), np.empty((height, w, 3), np.float32)
    var = np.empty((height, w), np.float32)
    check(lib.rt2_deinterleave_estimate_host(_fp(stacks), _fp(stacks2), _fp(image), _fp(mean), _fp(var), w, height,
                                             int(band_h), world, int(frames)))
    return image, mean, var


def deinterleave_adaptive(stacks: np.ndarray, stacks2: Optional[np.ndarray], counts: np.ndarray, height: int, band_h: int):
    """Rank-major padded band stacks (world, max_rows, W, 3) of the sums and (or None) of their squares, and
    (world, max_rows, W) uint32 of each pixel's sample count -> (sums, means, variance of the mean or None, counts) in
    image order: the host statement of the gather's kernel under adaptive sampling of the gathered image
    (rt2_deinterleave_adaptive_host), each pixel divided by its own count."""
    stacks = np.ascontiguousarray(stacks, np.float32)
    counts = np.ascontiguousarray(counts, np.uint32)
    world, max_rows, w, c = stacks.shape
    if stacks2 is not None:
        stacks2 = np.ascontiguousarray(stacks2, np.float32)
    if (c != 3 or counts.shape != (world, max_rows, w) or (stacks2 is not None and stacks2.shape != stacks.shape)
            or max_rows != band_rows_max(height, band_h, world)):
        raise ValueError("deinterleave_adaptive: need (world, band_rows_max, W, 3) stacks and (world, band_rows_max, W) counts")
    image, mean = np.empty((height, w, 3), np.float32), np.empty((height, w, 3), np.float32)
    var = np.empty((height, w), np.float32) if stacks2 is not None else None
    n = np.empty((height, w), np.uint32)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    check(lib.rt2_deinterleave_adaptive_host(_fp(stacks), _fp(stacks2) if stacks2 is not None else None,
                                             counts.ctypes.data_as(u32), _fp(image), _fp(mean),
                                             _fp(var) if var is not None else None, n.ctypes.data_as(u32), w, height,
                                             int(band_h), world))
    return image, mean, var, n


def source_rows(height: int, band_h: int, world: int) -> np.ndarray:
    """Image row y -> row of the rank-major padded stacks viewed as (world * max_rows) rows: the C
    ABI's host de-interleave applied to the stacks' own row numbers (one channel)."""
    max_rows = band_rows_max(height, band_h, world)
    ids = np.arange(world * max_rows, dtype=np.float32).reshape(world, max_rows, 1, 1)
    return deinterleave(ids, height, band_h)[:, 0, 0].astype(np.int64)


def combine_noise(parts) -> dict:
    """Merges the noise() dicts of tracers that each hold a part of one image (one process per GPU: the
    ranks' row bands) as a multi-GPU tracer's rt2_tracer_noise does, on the host: pixels, below,
    nonfinite and sum_sq add up (in list order), max_err is the largest, rms is recomputed as
    float32(sqrt(sum_sq / (pixels - nonfinite))), 0 when no pixel is finite. The parts must rest on the
    same frame count."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_noise: no parts")
    frames = {int(p["frames"]) for p in parts}
    if len(frames) != 1:
        raise ValueError(f"combine_noise: the parts rest on different frame counts {sorted(frames)}")
    out = {"frames": frames.pop(), "pixels": 0, "below": 0, "nonfinite": 0, "sum_sq": 0.0, "max_err": 0.0}
    for p in parts:
        for k in ("pixels", "below", "nonfinite"):
            out[k] += int(p[k])
        out["sum_sq"] = out["sum_sq"] + float(p["sum_sq"])
        out["max_err"] = max(out["max_err"], float(p["max_err"]))
    finite = out["pixels"] - out["nonfinite"]
    out["rms"] = float(np.float32(np.sqrt(np.float64(out["sum_sq"]) / np.float64(finite)))) if finite else 0.0
    return out


class BandGather:
    """Gathers (rows_r, W, C) float32 band stacks of every rank into one (H, W, C) image on rank 0:
    every rank sends its padded stack (band_rows_max rows) with one torch.distributed gather into a
    rank-major buffer (the layout ncclGather fills inside rt2_tracer_gather), which rank 0
    de-interleaves with one index_select on the buffer's device by the C ABI's row map
    (source_rows). The image stays where the stacks are: a device tensor for device buffers (no host
    copy), a host tensor for CPU ones."""

    def __init__(self, height: int, width: int, band_h: int, world: int, rank: int, device: torch.device,
                 channels: int = 3, group: Optional[dist.ProcessGroup] = None):
        self.height, self.width, self.band_h, self.world, self.rank = height, width, band_h, world, rank
        self.group = group
        self.rows = [local_rows(height, band_h, r, world) for r in range(world)]
        self.max_rows = band_rows_max(height, band_h, world)
        self.send = torch.zeros((self.max_rows, width, channels), dtype=torch.float32, device=device)
        self.stacks: Optional[torch.Tensor] = None
        self.image: Optional[torch.Tensor] = None
        if rank == 0:
            self.stacks = torch.zeros((world, self.max_rows, width, channels), dtype=torch.float32, device=device)
            self.image = torch.zeros((height, width, channels), dtype=torch.float32, device=device)
            self.src = torch.from_numpy(source_rows(height, band_h, world)).to(device)

    def local_view(self) -> torch.Tensor:
        """The part of the send buffer this rank fills (its local rows)."""
        return self.send[:len(self.rows[self.rank])]

    def gather(self) -> Optional[torch.Tensor]:
        """Collective: every rank calls it; rank 0 returns the assembled image (on the stacks' device),
        the others None."""
        if self.world == 1:
            self.stacks[0].copy_(self.send)
        else:
            recv: Optional[List[torch.Tensor]] = list(self.stacks.unbind(0)) if self.rank == 0 else None
            dist.gather(self.send, recv, dst=0, group=self.group)
            if self.rank != 0:
                return None
        flat = self.stacks.view(self.world * self.max_rows, self.width, -1)
        torch.index_select(flat, 0, self.src, out=self.image)
        return self.image
