"""Python mirror of the reference's hot-path interface, over the C ABI (include/rt2.h).

Names follow the reference so callers read the same:
  serialize::SceneLoader::LoadScene   (src/Serialize.hpp:21-31)  -> SceneLoader().LoadScene(path)
  serialize::LoadCamera / WriteCamera (src/Serialize.hpp:34-35)  -> LoadCamera(path), WriteCamera(cam, path)
  serialize::LoadAppSettings          (src/Serialize.hpp:33)     -> LoadAppSettings(path)
  cpu::RayTracer                      (src/cpu_raytrace/RayTracer.hpp:15-42) -> RayTracer
  util::WriteImage                    (src/Util.hpp:11-12)       -> WriteImage(pixels, w, h, path)
Everything here is host plumbing; the per-pixel render loop runs in the gfx950 kernel.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._native import AppSettings as _AppSettings
from ._native import (UNIQUE_ID_BYTES, Adaptive, CameraDesc, DenoiseParams, Noise, PresentParams, RadianceParams, SceneInfo,
                      Stats, TemporalParams, check, lib)

DEFAULT_SEED = 0x5EED2024
FLT_MAX = float(np.finfo(np.float32).max)
AMBIENT_INVALID = np.uint32(0xFFFFFFFF)  # ambient_counts / ambient_points: a miss pixel, an invalid point
RADIANCE_INVALID = np.uint32(0xFFFFFFFF)  # radiance(counts=True): the ray count of an invalid ray
RADIANCE_FRAME0 = 0x40000000  # radiance(streams=None): every ray's frame word (its pixel word is its row)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(t):
    """A torch tensor's device pointer."""
    return ctypes.c_void_p(t.data_ptr())


@dataclass
class Camera:
    """Camera parameters that the scene files carry (Camera.hpp:113-123; Serialize.cpp:32-38)."""
    center: Tuple[float, float, float] = (0.0, 0.0, 1.0)
    look_at: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    view_up: Tuple[float, float, float] = (0.0, 1.0, 0.0)
    vfov: float = 90.0
    defocus_angle: float = 0.0
    focus_distance: float = 1.0

    @classmethod
    def _from_desc(cls, d: CameraDesc) -> "Camera":
        return cls(tuple(d.center), tuple(d.look_at), tuple(d.view_up), d.vfov, d.defocus_angle, d.focus_distance)

    def _desc(self) -> CameraDesc:
        d = CameraDesc()
        d.center[:] = self.center
        d.look_at[:] = self.look_at
        d.view_up[:] = self.view_up
        d.vfov, d.defocus_angle, d.focus_distance = self.vfov, self.defocus_angle, self.focus_distance
        return d


@dataclass
class Settings:
    """AppSettings (src/Settings.hpp:5-11)."""
    render_once: bool = False
    save_after_render_once: bool = False
    num_samples: int = 1
    max_depth: int = 50
    render_window: bool = True


def LoadCamera(path: str) -> Camera:
    d = CameraDesc()
    check(lib.rt2_camera_load(path.encode(), ctypes.byref(d)))
    return Camera._from_desc(d)


def WriteCamera(cam: Camera, path: str) -> None:
    d = cam._desc()
    check(lib.rt2_camera_write(ctypes.byref(d), path.encode()))


def LoadAppSettings(path: str) -> Settings:
    s = _AppSettings()
    check(lib.rt2_settings_load(path.encode(), ctypes.byref(s)))
    return Settings(bool(s.render_once), bool(s.save_after_render_once), int(s.num_samples), int(s.max_depth),
                    bool(s.render_window))


def WriteImage(pixels: np.ndarray, width: int, height: int, path: str, png: bool = True) -> None:
    """util::WriteImage: `pixels` float32 (height, width, 3), row 0 = bottom row."""
    p = np.ascontiguousarray(pixels, dtype=np.float32)
    if p.size != width * height * 3:
        raise ValueError("pixels must hold width*height*3 floats")
    check(lib.rt2_write_image(_fp(p), width, height, path.encode(), 1 if png else 0))


class Scene:
    """A loaded + compiled scene (cpu::Scene after App.cpp:126 wraps the list in one BVHNode)."""

    def __init__(self, path: str, seed: int = DEFAULT_SEED):
        h = ctypes.c_void_p()
        check(lib.rt2_scene_load(path.encode(), seed, ctypes.byref(h)))
        self._h = h
        self.path = path
        self.seed = seed

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib.rt2_scene_free(self._h)
            self._h = None

    def info(self) -> SceneInfo:
        s = SceneInfo()
        check(lib.rt2_scene_get_info(self._h, ctypes.byref(s)))
        return s

    @property
    def dims(self) -> Tuple[int, int]:
        i = self.info()
        return i.dims_x, i.dims_y

    @property
    def background_color(self) -> Tuple[float, float, float]:
        return tuple(self.info().background)

    def materials(self) -> np.ndarray:
        n = check(lib.rt2_scene_materials(self._h, None, 0))
        out = np.zeros((max(n, 1), 8), np.float32)
        check(lib.rt2_scene_materials(self._h, _fp(out), n))
        return out[:n]

    def textures(self) -> np.ndarray:
        n = check(lib.rt2_scene_textures(self._h, None, 0))
        out = np.zeros((max(n, 1), 8), np.float32)
        check(lib.rt2_scene_textures(self._h, _fp(out), n))
        return out[:n]

    def perlin(self, tex: int):
        pc = check(lib.rt2_scene_perlin(self._h, tex, None, None))
        vec = np.zeros((pc, 3), np.float32)
        perm = np.zeros(3 * pc, np.int32)
        check(lib.rt2_scene_perlin(self._h, tex, _fp(vec), perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return vec, perm.reshape(3, pc)

    @property
    def cam(self) -> Camera:
        d = CameraDesc()
        check(lib.rt2_scene_get_camera(self._h, ctypes.byref(d)))
        return Camera._from_desc(d)

    @cam.setter
    def cam(self, c: Camera) -> None:
        d = c._desc()
        check(lib.rt2_scene_set_camera(self._h, ctypes.byref(d)))

    def camera_params(self, w: int, h: int, spp: int) -> np.ndarray:
        out = np.zeros(21, np.float32)
        check(lib.rt2_camera_params(self._h, w, h, spp, _fp(out)))
        return out


class SceneLoader:
    """serialize::SceneLoader: LoadScene returns a Scene, or None (std::nullopt) with `.error` set."""

    def __init__(self, seed: int = DEFAULT_SEED):
        self.seed = seed
        self.error: Optional[str] = None

    def LoadScene(self, filepath: str) -> Optional[Scene]:
        try:
            self.error = None
            return Scene(filepath, self.seed)
        except RuntimeError as e:
            self.error = str(e)
            return None


def band_rank(band: int, world: int) -> int:
    """Rank owning row band `band` (rt2_layout.h BandRank): period p = band // world, phase
    q = band % world, rank (q + p) % world — one band per period per rank, phases rotating."""
    return (band % world + band // world) % world


def local_rows(height: int, band_h: int, rank: int, world: int) -> List[int]:
    """Global rows owned by `rank` under the interleaved row-band partition, in increasing y."""
    bh = band_h if band_h > 0 else height
    return [y for y in range(height) if band_rank(y // bh, world) == rank]


def assemble_bands(parts: Sequence[np.ndarray], height: int, band_h: int) -> np.ndarray:
    """Inverse of the partition: parts[r] holds rank r's local rows (n_r, W, C) in increasing y."""
    world = len(parts)
    w = parts[0].shape[1]
    out = np.zeros((height, w) + parts[0].shape[2:], parts[0].dtype)
    for r, p in enumerate(parts):
        rows = local_rows(height, band_h, r, world)
        out[rows] = p[:len(rows)]
    return out


def comm_unique_id() -> bytes:
    """rt2_comm_unique_id: the RCCL id rank 0 makes and the caller broadcasts before join()."""
    buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES)()
    check(lib.rt2_comm_unique_id(buf, UNIQUE_ID_BYTES))
    return bytes(buf)


def denoise_defaults() -> dict:
    """rt2_denoise_defaults as a dict."""
    p = DenoiseParams()
    lib.rt2_denoise_defaults(ctypes.byref(p))
    return p.as_dict()


def _denoise_params(params: dict):
    """A rt2_denoise_params pointer for the keyword arguments (None = NULL: the defaults)."""
    if not params:
        return None
    p = DenoiseParams()
    lib.rt2_denoise_defaults(ctypes.byref(p))
    for k, v in params.items():
        if k not in dict(DenoiseParams._fields_):
            raise TypeError(f"denoise: unknown parameter {k!r}")
        setattr(p, k, int(v) if k in ("iterations", "normal_power_log2") else float(v))
    return ctypes.byref(p)


def denoise_buffers(color, variance, features, device: int = 0, **params):
    """rt2_denoise_buffers: the tracer's filter over caller buffers, color (H, W, 3), variance (H, W),
    features (H, W, 16) float32. Returns (color', variance')."""
    color = np.ascontiguousarray(color, np.float32)
    variance = np.ascontiguousarray(variance, np.float32)
    features = np.ascontiguousarray(features, np.float32)
    h, w = variance.shape
    if color.shape != (h, w, 3) or features.shape != (h, w, 16):
        raise ValueError("denoise_buffers: need color (H, W, 3), variance (H, W), features (H, W, 16)")
    out, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    check(lib.rt2_denoise_buffers(int(device), w, h, _fp(color), _fp(variance), _fp(features), _denoise_params(params),
                                  _fp(out), _fp(var)))
    return out, var


def temporal_defaults() -> dict:
    """rt2_temporal_defaults as a dict."""
    p = TemporalParams()
    lib.rt2_temporal_defaults(ctypes.byref(p))
    return p.as_dict()


def _temporal_params(params: dict):
    """A rt2_temporal_params pointer for the keyword arguments (None = NULL: the defaults)."""
    if not params:
        return None
    p = TemporalParams()
    lib.rt2_temporal_defaults(ctypes.byref(p))
    for k, v in params.items():
        if k not in dict(TemporalParams._fields_):
            raise TypeError(f"temporal: unknown parameter {k!r}")
        setattr(p, k, float(v))
    return ctypes.byref(p)


def temporal_buffers(color, variance, length, features, hist_color, hist_variance, hist_length, hist_features, hist_camera,
                     materials=None, device: int = 0, **params):
    """rt2_temporal_buffers: the tracer's temporal blend over caller buffers: the current and the history's color
    (H, W, 3), variance (H, W), length (H, W), features (H, W, 16) float32, the 21 camera words the history was
    taken under, and the material table (n, 8) of Scene.materials() or None. Returns (color', variance', length')."""
    cur = [np.ascontiguousarray(a, np.float32) for a in (color, variance, length, features)]
    old = [np.ascontiguousarray(a, np.float32) for a in (hist_color, hist_variance, hist_length, hist_features)]
    cam = np.ascontiguousarray(hist_camera, np.float32)
    if cur[1].ndim != 2:
        raise ValueError("temporal_buffers: need variance (H, W)")
    h, w = cur[1].shape
    shapes = [(h, w, 3), (h, w), (h, w), (h, w, 16)]
    if [a.shape for a in cur] != shapes or [a.shape for a in old] != shapes or cam.shape != (21,):
        raise ValueError("temporal_buffers: need color (H, W, 3), variance (H, W), length (H, W), features (H, W, 16) of the "
                         "current image and of the history, and 21 camera words")
    mats, n_mats = None, 0
    if materials is not None:
        mats = np.ascontiguousarray(materials, np.float32)
        if mats.ndim != 2 or mats.shape[1] != 8:
            raise ValueError("temporal_buffers: need materials (n, 8)")
        n_mats = mats.shape[0]
    out, var, ln = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    check(lib.rt2_temporal_buffers(int(device), w, h, *[_fp(a) for a in cur], *[_fp(a) for a in old], _fp(cam),
                                   _fp(mats) if n_mats else None, n_mats, _temporal_params(params), _fp(out), _fp(var),
                                   _fp(ln)))
    return out, var, ln


def present_defaults() -> dict:
    """rt2_present_defaults as a dict: temporal, denoise, tp (temporal_defaults()), dp (denoise_defaults())."""
    p = PresentParams()
    lib.rt2_present_defaults(ctypes.byref(p))
    return p.as_dict()


def _present_params(params: dict):
    """A rt2_present_params pointer for the keyword arguments of RayTracer.present (None = NULL: the defaults):
    temporal, denoise (switches) and tp, dp (dicts of the rt2_temporal_params / rt2_denoise_params fields that
    differ from the defaults)."""
    if not params:
        return None
    p = PresentParams()
    lib.rt2_present_defaults(ctypes.byref(p))
    for k, v in params.items():
        if k in ("temporal", "denoise"):
            setattr(p, k, 1 if v else 0)
        elif k == "tp":
            for f, x in (v or {}).items():
                if f not in dict(TemporalParams._fields_):
                    raise TypeError(f"present: unknown temporal parameter {f!r}")
                setattr(p.tp, f, float(x))
        elif k == "dp":
            for f, x in (v or {}).items():
                if f not in dict(DenoiseParams._fields_):
                    raise TypeError(f"present: unknown denoise parameter {f!r}")
                setattr(p.dp, f, int(x) if f in ("iterations", "normal_power_log2") else float(x))
        else:
            raise TypeError(f"present: unknown parameter {k!r}")
    return ctypes.byref(p)


def ray_valid(rays) -> np.ndarray:
    """rt2_query_ray_valid for each of rays (n, 8) float32 (one ray: (8,)): whether intersect() traces it (all
    words finite, 0.001 < tmax, 0 <= time <= 1, origin within +-2^64, the direction's largest component within
    [2^-20, 2^20]) or answers -1. Returns (n,) bool."""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    return np.array([bool(lib.rt2_query_ray_valid(_fp(r[i:i + 1]))) for i in range(len(r))], bool)


def present_buffers(color, device: int = 0) -> np.ndarray:
    """rt2_present_buffers: the tone map of present() over a caller image, color (H, W, 3) float32, on `device`.
    Returns (H, W, 4) uint8."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise ValueError("present_buffers: need color (H, W, 3)")
    h, w = color.shape[:2]
    out = np.zeros((h, w, 4), np.uint8)
    check(lib.rt2_present_buffers(int(device), w, h, _fp(color), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    return out


class RayTracer:
    """cpu::RayTracer (RayTracer.hpp:15-42) on one or more MI355X GPUs.

    Update() renders one frame (one sample per pixel) exactly like RayTracer::Update; Render(n) is
    n Update() calls in one kernel launch. Image buffers hold this tracer's local rows (all rows
    unless set_partition()/join() was called). With `n_gpus` or `devices` the tracer renders on
    several GPUs of this process (rt2_tracer_create_multi: interleaved row bands, RCCL gather) and
    its readbacks return the full image.

    `camera`, like the reference's borrowed `Camera* camera` (RayTracer.hpp:31), is read at every
    Update()/Render() when set: a moved camera applies from the next frame (RayTracer.cpp:56).
    """

    def __init__(self, scene: Scene, device: int = 0, *, n_gpus: Optional[int] = None,
                 devices: Optional[Sequence[int]] = None, band_h: int = 0):
        h = ctypes.c_void_p()
        if n_gpus is None and devices is None:
            check(lib.rt2_tracer_create(scene._h, device, ctypes.byref(h)))
            self.devices = [device]
        else:
            devs = list(devices) if devices is not None else list(range(device, device + int(n_gpus)))
            arr = (ctypes.c_int * len(devs))(*devs)
            check(lib.rt2_tracer_create_multi(scene._h, len(devs), arr, int(band_h), ctypes.byref(h)))
            self.devices = devs
        self._h = h
        self.device = self.devices[0]
        self._max_depth = 50
        self._moments = False
        self._seed = DEFAULT_SEED  # the tracer's seed (rt2_tracer_set_seed), intersect()'s default
        self.camera: Optional[Camera] = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib.rt2_tracer_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # -- reference members ------------------------------------------------------------------
    @property
    def max_depth(self) -> int:
        return self._max_depth

    @max_depth.setter
    def max_depth(self, d: int) -> None:
        check(lib.rt2_tracer_set_max_depth(self._h, int(d)))
        self._max_depth = int(d)

    def SetSamplesPerPixel(self, spp: int) -> None:
        """scene.cam.SetSamplesPerPixel(settings.num_samples) (App.cpp:129): fixes the strata."""
        check(lib.rt2_tracer_set_samples_per_pixel(self._h, int(spp)))

    def OnResize(self, dims: Tuple[int, int]) -> None:
        check(lib.rt2_tracer_on_resize(self._h, int(dims[0]), int(dims[1])))

    def Reset(self) -> None:
        check(lib.rt2_tracer_reset(self._h))

    def _push_camera(self) -> None:
        if self.camera is not None:
            self.set_camera(self.camera)

    def Update(self, scene: Optional[Scene] = None) -> None:
        self._push_camera()  # camera->Update() (RayTracer.cpp:56)
        check(lib.rt2_tracer_update(self._h))

    def Render(self, n_frames: int) -> None:
        self._push_camera()
        check(lib.rt2_tracer_render(self._h, int(n_frames)))

    def FrameIdx(self) -> int:
        return int(lib.rt2_tracer_frame_idx(self._h))

    def Dims(self) -> Tuple[int, int]:
        w, h = ctypes.c_int(), ctypes.c_int()
        check(lib.rt2_tracer_dims(self._h, ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def local_rows(self) -> int:
        return int(lib.rt2_tracer_local_rows(self._h))

    def NonConvertedPixels(self) -> np.ndarray:
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w, 3), np.float32)
        check(lib.rt2_tracer_non_converted_pixels(self._h, _fp(out)))
        return out

    def Accumulation(self) -> np.ndarray:
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w, 3), np.float32)
        check(lib.rt2_tracer_accumulation(self._h, _fp(out)))
        return out

    def Pixels(self) -> np.ndarray:
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w, 4), np.uint8)
        check(lib.rt2_tracer_pixels(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    # -- MI355X extensions ------------------------------------------------------------------
    def set_camera(self, cam: Camera) -> None:
        """rt2_tracer_set_camera: the camera's setter fields for the next frames (queued frames
        keep the camera they were queued under; the accumulation is not reset)."""
        d = cam._desc()
        check(lib.rt2_tracer_set_camera(self._h, ctypes.byref(d)))

    def get_camera(self) -> Camera:
        d = CameraDesc()
        check(lib.rt2_tracer_get_camera(self._h, ctypes.byref(d)))
        return Camera._from_desc(d)

    def n_gpus(self) -> int:
        return int(check(lib.rt2_tracer_n_gpus(self._h)))

    def join(self, unique_id: bytes, world: int, rank: int, band_h: int = 0) -> None:
        """rt2_tracer_join: partition (band_h, rank, world) + this rank of an RCCL communicator."""
        buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id[:UNIQUE_ID_BYTES])
        check(lib.rt2_tracer_join(self._h, buf, int(world), int(rank), int(band_h)))

    def gather(self) -> None:
        """rt2_tracer_gather: collective; the full image lands on rank 0 (enqueued, no wait)."""
        check(lib.rt2_tracer_gather(self._h))

    def image_accumulation(self) -> np.ndarray:
        w, h = self.Dims()
        out = np.zeros((h, w, 3), np.float32)
        check(lib.rt2_tracer_image_accumulation(self._h, _fp(out)))
        return out

    def image_non_converted_pixels(self) -> np.ndarray:
        w, h = self.Dims()
        out = np.zeros((h, w, 3), np.float32)
        check(lib.rt2_tracer_image_non_converted_pixels(self._h, _fp(out)))
        return out

    def image_pixels(self) -> np.ndarray:
        w, h = self.Dims()
        out = np.zeros((h, w, 4), np.uint8)
        check(lib.rt2_tracer_image_pixels(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def set_seed(self, seed: int) -> None:
        check(lib.rt2_tracer_set_seed(self._h, int(seed)))
        self._seed = int(seed)

    def set_partition(self, band_h: int, rank: int, world: int) -> None:
        check(lib.rt2_tracer_set_partition(self._h, int(band_h), int(rank), int(world)))

    def set_launch_frames(self, n: int) -> None:
        check(lib.rt2_tracer_set_launch_frames(self._h, int(n)))

    def flush(self) -> None:
        """Launch the queued Update()/Render() frames now (does not wait for them)."""
        check(lib.rt2_tracer_flush(self._h))

    def query(self) -> int:
        """1 when every GPU has finished the work enqueued so far, 0 while some is still running
        (launches queued frames first, like flush(); never waits)."""
        r = lib.rt2_tracer_query(self._h)
        if r < 0:
            check(r)
        return r

    def set_lazy_frames(self, max_queued: int) -> None:
        check(lib.rt2_tracer_set_lazy_frames(self._h, int(max_queued)))

    def set_work_split(self, items_per_lane: int) -> None:
        check(lib.rt2_tracer_set_work_split(self._h, int(items_per_lane)))

    def set_sample_budget(self, nbytes: int) -> None:
        check(lib.rt2_tracer_set_sample_budget(self._h, int(nbytes)))

    def set_batch_max(self, items: int) -> None:
        check(lib.rt2_tracer_set_batch_max(self._h, int(items)))

    def last_launch(self) -> dict:
        g, c, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib.rt2_tracer_last_launch(self._h, ctypes.byref(g), ctypes.byref(c), ctypes.byref(v)))
        return {"grid": g.value, "chunk_frames": c.value, "variant": v.value}

    def set_stream(self, hip_stream_ptr: Optional[int]) -> None:
        check(lib.rt2_tracer_set_stream(self._h, ctypes.c_void_p(hip_stream_ptr or None)))

    def synchronize(self) -> None:
        check(lib.rt2_tracer_synchronize(self._h))

    def copy_accum_to(self, dst_ptr: int, stream_ptr: Optional[int] = None) -> None:
        check(lib.rt2_tracer_copy_accum_device(self._h, ctypes.c_void_p(dst_ptr), ctypes.c_void_p(stream_ptr or None)))

    def enable_ray_counts(self, on: bool = True) -> None:
        check(lib.rt2_tracer_enable_ray_counts(self._h, 1 if on else 0))

    def ray_counts(self) -> np.ndarray:
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w), np.uint32)
        check(lib.rt2_tracer_ray_counts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    # -- noise estimate (rt2.h "Noise estimate and render-until-converged") -------------------
    def enable_moments(self, on: bool = True) -> None:
        """Sums of the samples' squares beside the accumulation, in frame order (resets the frame)."""
        check(lib.rt2_tracer_enable_moments(self._h, 1 if on else 0))
        self._moments = bool(on)

    def moments(self) -> np.ndarray:
        """Raw float3 sums of squares per local pixel (a multi-GPU tracer: the full image)."""
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w, 3), np.float32)
        check(lib.rt2_tracer_moments(self._h, _fp(out)))
        return out

    def standard_error(self) -> np.ndarray:
        """Float3 standard error of the mean per local pixel (needs FrameIdx() >= 2)."""
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w, 3), np.float32)
        check(lib.rt2_tracer_standard_error(self._h, _fp(out)))
        return out

    def noise(self, threshold: float = 0.0) -> dict:
        """rt2_noise as a dict: frames, pixels, below (err <= threshold), nonfinite, sum_sq, max_err, rms."""
        n = Noise()
        check(lib.rt2_tracer_noise(self._h, float(threshold), ctypes.byref(n)))
        return n.as_dict()

    def render_until(self, target_rms: float, max_frames: int, min_frames: int = 0, check_every: int = 0) -> dict:
        """Renders in steps of check_every frames (0: one stratum sweep) until the image's rms noise is at
        most target_rms or FrameIdx() reaches max_frames; returns the last estimate (noise())."""
        self._push_camera()
        n = Noise()
        check(lib.rt2_tracer_render_until(self._h, float(target_rms), int(min_frames), int(max_frames),
                                          int(check_every), ctypes.byref(n)))
        return n.as_dict()

    # -- adaptive sampling (rt2.h "Adaptive sampling") ----------------------------------------
    def enable_adaptive(self, on: bool = True) -> None:
        """Retire converged pixels and render only the rest (needs enable_moments; resets the frame)."""
        check(lib.rt2_tracer_enable_adaptive(self._h, 1 if on else 0))

    def sample_counts(self) -> np.ndarray:
        """uint32 sample count n_p per local pixel."""
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w), np.uint32)
        check(lib.rt2_tracer_sample_counts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def adaptive_check(self, threshold: float, window: int = 1) -> dict:
        """Retires the active pixels with no pixel over `threshold` within `window` columns of their row;
        rt2_adaptive as a dict: frames, pixels, active, retired, samples, nonfinite."""
        a = Adaptive()
        check(lib.rt2_tracer_adaptive_check(self._h, float(threshold), int(window), ctypes.byref(a)))
        return a.as_dict()

    def render_adaptive(self, threshold: float, max_frames: int, window: int = 1, min_frames: int = 0,
                        check_every: int = 0) -> dict:
        """Renders in steps of check_every frames (0: one stratum sweep) with a check after each, until no
        pixel is active or FrameIdx() reaches max_frames; returns the last check (adaptive_check())."""
        self._push_camera()
        a = Adaptive()
        check(lib.rt2_tracer_render_adaptive(self._h, float(threshold), int(window), int(min_frames),
                                             int(max_frames), int(check_every), ctypes.byref(a)))
        return a.as_dict()

    # -- feature buffers and denoiser (rt2.h "Feature buffers and denoiser") -------------------
    def features(self) -> np.ndarray:
        """The first-hit record of the ray through each local pixel's centre, (rows, W, 16) float32: hit, t,
        point, normal, front_face, material, albedo, dist, 0, 0 (cached on the device per camera)."""
        self._push_camera()
        w, _ = self.Dims()
        out = np.zeros((self.local_rows(), w, 16), np.float32)
        check(lib.rt2_tracer_features(self._h, _fp(out)))
        return out

    def denoise(self, variance: bool = False, **params):
        """The variance-guided a-trous filter over the mean image (needs enable_moments, FrameIdx() >= 2, one
        unpartitioned GPU): (H, W, 3) float32, with variance=True also the filtered variance of the mean
        (H, W). params: the fields of rt2_denoise_params that differ from denoise_defaults()."""
        self._push_camera()
        w, _ = self.Dims()
        rows = max(self.local_rows(), 0)
        out = np.zeros((rows, w, 3), np.float32)
        var = np.zeros((rows, w), np.float32) if variance else None
        check(lib.rt2_tracer_denoise(self._h, _denoise_params(params), _fp(out), _fp(var) if variance else None))
        return (out, var) if variance else out

    def denoise_times(self) -> dict:
        """GPU ms of the last feature pass and of the last denoise call's kernels (-1: none yet)."""
        f, d = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        check(lib.rt2_tracer_denoise_times(self._h, ctypes.byref(f), ctypes.byref(d)))
        return {"features_ms": f.value, "denoise_ms": d.value}

    # -- ray queries (rt2.h "Ray queries") -------------------------------------------------------
    def _batch(self, batch, what: str, call: str):
        """The (n, 8) float32 batch of a query (`what`: "rays" or "points") made contiguous, and whether it is a CUDA
        torch tensor on the tracer's device, which goes through the call's device entry, or a numpy array, which
        goes through its host entry."""
        if not isinstance(batch, np.ndarray) and hasattr(batch, "is_cuda"):
            import torch
            if not batch.is_cuda or batch.device.index != self.device:
                raise ValueError(f"{call}: need a tensor on cuda:{self.device}")
            if batch.dtype != torch.float32 or batch.dim() != 2 or batch.shape[1] != 8:
                raise ValueError(f"{call}: need {what} (n, 8) float32")
            return batch.contiguous(), True
        batch = np.ascontiguousarray(batch, np.float32)
        if batch.ndim != 2 or batch.shape[1] != 8:
            raise ValueError(f"{call}: need {what} (n, 8) float32")
        return batch, False

    def _device_call(self, fn, batch, *args) -> None:
        """fn(tracer, n, batch, *args), a device entry, complete on return (nothing to do for an empty batch): the
        current stream has written the batch and allocated the outputs before it, the tracer's has run it after."""
        if batch.shape[0] == 0:
            return
        import torch
        torch.cuda.current_stream(batch.device).synchronize()
        check(fn(self._h, batch.shape[0], _dp(batch), *args))
        self.synchronize()

    def _ms(self, fn) -> float:
        """A *_time getter: fn's GPU ms."""
        ms = ctypes.c_double(-1.0)
        check(fn(self._h, ctypes.byref(ms)))
        return ms.value

    def intersect(self, rays, seed: Optional[int] = None):
        """The scene's closest hit for rays of the caller: rays (n, 8) float32, ox oy oz tmax dx dy dz time ->
        (n, 16) float32 in the feature record's layout, slot 0 = 1 hit, 0 miss, -1 not traced (ray_valid). seed
        keys a ConstantMedium's draws (default: the tracer's seed). A numpy array goes through the host entry
        (queued frames are launched first) and a numpy array comes back; a CUDA torch tensor on the tracer's
        device goes through the device entry into a new tensor, complete on return."""
        seed = self._seed if seed is None else int(seed)
        rays, on_device = self._batch(rays, "rays", "intersect")
        n = rays.shape[0]
        if on_device:
            import torch
            out = torch.empty((n, 16), dtype=torch.float32, device=rays.device)
            self._device_call(lib.rt2_tracer_intersect_device, rays, seed, _dp(out))
            return out
        out = np.zeros((n, 16), np.float32)
        if n:
            check(lib.rt2_tracer_intersect(self._h, n, _fp(rays), seed, _fp(out)))
        return out

    def occluded(self, rays, seed: Optional[int] = None):
        """Whether anything lies in (0.001, tmax) along rays of the caller: rays (n, 8) float32 as intersect's ->
        (n,) int8, 1 occluded, 0 clear, -1 not traced (ray_valid): slot 0 of intersect's record for the same ray and
        seed, from a walk that ends at its first hit and resolves nothing. A numpy array goes through the host
        entry and a numpy array comes back; a CUDA torch tensor on the tracer's device goes through the device
        entry into a new int8 tensor, complete on return."""
        seed = self._seed if seed is None else int(seed)
        rays, on_device = self._batch(rays, "rays", "occluded")
        n = rays.shape[0]
        if on_device:
            import torch
            out = torch.empty((n,), dtype=torch.int8, device=rays.device)
            self._device_call(lib.rt2_tracer_occluded_device, rays, seed, _dp(out))
            return out
        out = np.zeros((n,), np.int8)
        if n:
            check(lib.rt2_tracer_occluded(self._h, n, _fp(rays), seed, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))))
        return out

    def visible(self, a, b, time: float = 0.0, seed: Optional[int] = None) -> np.ndarray:
        """Whether the segment from a[i] to b[i] is clear, points (n, 3): (n,) int8, 1 visible, 0 blocked, -1 not
        traced (a == b, or a segment outside ray_valid's domain). The ray is o = a, d = b - a (one float32
        subtraction per component) over the interval (0.001, 0.999): both margins are fractions of the segment,
        not distances, so a surface within a thousandth of the segment's length of either end point does not
        block it. The answer is the reference's Hit on that interval, with its quirk: a transformed child compares
        its model-space t, taken along the normalised direction, with the same 0.999, so it blocks a segment
        only where that t is below 0.999. Where transformed geometry must block, call occluded() with a unit
        direction and tmax = the distance, which both kinds of children read alike."""
        a = np.asarray(a, np.float32).reshape(-1, 3)
        b = np.asarray(b, np.float32).reshape(-1, 3)
        if a.shape != b.shape:
            raise ValueError("visible: need as many points b as points a")
        rays = np.zeros((len(a), 8), np.float32)
        rays[:, 0:3] = a
        rays[:, 3] = np.float32(0.999)
        rays[:, 4:7] = b - a
        rays[:, 7] = np.float32(time)
        occ = self.occluded(rays, seed)
        return np.where(occ < 0, np.int8(-1), np.int8(1) - occ).astype(np.int8)

    def intersect_time(self) -> float:
        """GPU ms of the last query's kernels, intersect's or occluded's (-1: not finished yet, or none). Never
        waits."""
        return self._ms(lib.rt2_tracer_intersect_time)

    # -- ambient occlusion (rt2.h "Ambient occlusion") ---------------------------------------------
    def ambient_counts(self, samples: int, radius: float = FLT_MAX, seed: Optional[int] = None) -> np.ndarray:
        """Per local pixel the number of `samples` cosine-weighted occlusion rays from its first hit (features())
        that are blocked within `radius`: (rows, W) uint32, 0xFFFFFFFF where the pixel's ray missed. Drawn and
        traced on the GPU by the rule of rt2.h "Ambient occlusion"; seed (default: the tracer's) keys the samples,
        a ConstantMedium's draws and the feature pass. A readback: queued frames are launched first."""
        self._push_camera()
        seed = self._seed if seed is None else int(seed)
        w, _ = self.Dims()
        out = np.zeros((max(self.local_rows(), 0), w), np.uint32)
        check(lib.rt2_tracer_ambient(self._h, int(samples), float(radius), seed,
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def ambient(self, samples: int, radius: float = FLT_MAX, seed: Optional[int] = None) -> np.ndarray:
        """The visibility 1 - count / samples of ambient_counts() in float32, (rows, W); 1.0 where the pixel's
        ray missed."""
        c = self.ambient_counts(samples, radius, seed)
        vis = np.float32(1) - c.astype(np.float32) / np.float32(samples)
        return np.where(c == AMBIENT_INVALID, np.float32(1), vis).astype(np.float32)

    def ambient_points(self, points, samples: int, seed: Optional[int] = None):
        """The blocked-sample counts of caller points: points (n, 8) float32, px py pz tmax nx ny nz time ->
        (n,) uint32, 0xFFFFFFFF for a point outside ray_valid's domain (the normal as the direction). The stream
        index of a point is its row. A numpy array goes through the host entry and a numpy array comes back; a CUDA
        torch tensor on the tracer's device goes through the device entry into a new int32 tensor holding the
        uint32 words, complete on return."""
        seed = self._seed if seed is None else int(seed)
        points, on_device = self._batch(points, "points", "ambient_points")
        n = points.shape[0]
        if on_device:
            import torch
            out = torch.empty((n,), dtype=torch.int32, device=points.device)
            self._device_call(lib.rt2_tracer_ambient_points_device, points, int(samples), seed, _dp(out))
            return out
        out = np.zeros((n,), np.uint32)
        if n:
            check(lib.rt2_tracer_ambient_points(self._h, n, _fp(points), int(samples), seed,
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def ambient_time(self) -> float:
        """GPU ms of the last ambient call's kernels (-1: not finished yet, or none). Never waits."""
        return self._ms(lib.rt2_tracer_ambient_time)

    # -- radiance queries (rt2.h "Radiance queries") -----------------------------------------------
    def radiance(self, rays, samples: int = 1, streams=None, max_depth: Optional[int] = None, first_draw: int = 0,
                 seed: Optional[int] = None, counts: bool = False):
        """The radiance RayColor returns along rays of the caller, summed over `samples` paths per ray: rays (n, 8)
        float32 as intersect's -> (n, 3) float32 sums in sample order (divide by samples for the mean); with counts
        also (n,) uint32, the rays cast (0xFFFFFFFF and a zero sum for a ray outside ray_valid's domain). streams:
        (n, 2) uint32 (pixel word, frame word) per ray, default (row, 0x40000000); sample s draws from the path stream
        (seed, pixel word, frame word + s) after its first first_draw uniforms. max_depth: default the tracer's.
        With a camera's own ray, (y * W + x, f) and first_draw 3 (5 with defocus) the answer is that pixel's sample
        of frame f in a render, bit for bit. A numpy array goes through the host entry and numpy comes back; a CUDA
        torch tensor on the tracer's device (streams then a CUDA int32 tensor of the uint32 words, or None) goes
        through the device entry into new tensors (counts: int32 holding the uint32 words), complete on return."""
        seed = self._seed if seed is None else int(seed)
        prm = RadianceParams(int(samples), 0 if max_depth is None else int(max_depth), int(first_draw))
        if max_depth is not None and int(max_depth) < 1:
            raise ValueError("radiance: need max_depth >= 1 (None: the tracer's)")
        rays, on_device = self._batch(rays, "rays", "radiance")
        n = rays.shape[0]
        if on_device:
            import torch
            if streams is not None:
                if (not hasattr(streams, "is_cuda") or not streams.is_cuda or streams.device != rays.device or
                        streams.dtype != torch.int32 or tuple(streams.shape) != (n, 2)):
                    raise ValueError("radiance: need streams (n, 2) int32 on the rays' device")
                streams = streams.contiguous()
            out = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
            cnt = torch.empty((n,), dtype=torch.int32, device=rays.device) if counts else None
            self._device_call(lib.rt2_tracer_radiance_device, rays, _dp(streams) if streams is not None else None,
                              ctypes.byref(prm), seed, _dp(out), _dp(cnt) if counts else None)
            return (out, cnt) if counts else out
        u32p = ctypes.POINTER(ctypes.c_uint32)
        sp = None
        if streams is not None:
            streams = np.ascontiguousarray(streams, np.uint32)
            if streams.shape != (n, 2):
                raise ValueError("radiance: need streams (n, 2) uint32")
            sp = streams.ctypes.data_as(u32p)
        out = np.zeros((n, 3), np.float32)
        cnt = np.zeros((n,), np.uint32)
        if n:
            check(lib.rt2_tracer_radiance(self._h, n, _fp(rays), sp, ctypes.byref(prm), seed, _fp(out),
                                          cnt.ctypes.data_as(u32p) if counts else None))
        return (out, cnt) if counts else out

    def radiance_time(self) -> float:
        """GPU ms of the last radiance call's kernels (-1: not finished yet, or none). Never waits."""
        return self._ms(lib.rt2_tracer_radiance_time)

    # -- temporal reuse (rt2.h "Temporal reuse") ------------------------------------------------
    def temporal_resolve(self, denoise=False, variance: bool = False, length: bool = False, **params):
        """The current estimate blended with the history pushed before the last camera move (needs what denoise()
        needs): (H, W, 3) float32; with variance / length also the variance of the mean and the length in frames,
        (H, W) each. denoise: True, or a dict of rt2_denoise_params fields, runs denoise()'s filter over the blend.
        params: the fields of rt2_temporal_params that differ from temporal_defaults(). Changes nothing."""
        self._push_camera()
        w, _ = self.Dims()
        rows = max(self.local_rows(), 0)
        out = np.zeros((rows, w, 3), np.float32)
        var = np.zeros((rows, w), np.float32) if variance else None
        ln = np.zeros((rows, w), np.float32) if length else None
        dn = _denoise_params(denoise) if isinstance(denoise, dict) else None
        check(lib.rt2_tracer_temporal_resolve(self._h, _temporal_params(params), 1 if denoise else 0, dn, _fp(out),
                                              _fp(var) if variance else None, _fp(ln) if length else None))
        res = (out,) + ((var,) if variance else ()) + ((ln,) if length else ())
        return res if len(res) > 1 else out

    def temporal_push(self, **params) -> None:
        """Make the blended estimate (never filtered) the history, with the current features and camera: call it
        before changing the camera, then Reset()."""
        self._push_camera()
        check(lib.rt2_tracer_temporal_push(self._h, _temporal_params(params)))

    def temporal_clear(self) -> None:
        check(lib.rt2_tracer_temporal_clear(self._h))

    def temporal_time(self) -> float:
        """GPU ms of the last temporal_resolve's temporal kernels (-1: none yet)."""
        return self._ms(lib.rt2_tracer_temporal_time)

    # -- presenting reconstructed frames (rt2.h "Presenting reconstructed frames") ---------------
    def present(self, **params) -> np.ndarray:
        """The reconstructed frame as RGBA8, (H, W, 4) uint8: the estimate blended with the history (temporal,
        default on), filtered (denoise, default on) and tone-mapped like Pixels(). Needs what temporal_resolve()
        needs. params: temporal, denoise (switches), tp, dp (dicts of temporal / denoise parameter fields).
        Changes nothing."""
        self._push_camera()
        w, _ = self.Dims()
        out = np.zeros((max(self.local_rows(), 0), w, 4), np.uint8)
        check(lib.rt2_tracer_present(self._h, _present_params(params), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def present_async(self, pinned_array: np.ndarray, **params) -> None:
        """present() enqueued into `pinned_array` ((H, W, 4) uint8 of a progressive.PinnedBuffer), returning at
        once: the bytes are complete after synchronize() or once query() returns 1."""
        w, _ = self.Dims()
        a = pinned_array
        if a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"] or a.nbytes != max(self.local_rows(), 0) * w * 4:
            raise ValueError("present_async: need a C-contiguous uint8 array of H * W * 4 bytes")
        self._push_camera()
        check(lib.rt2_tracer_present_async(self._h, _present_params(params), a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def move_camera(self, cam: Camera, **temporal_params) -> None:
        """temporal_push(), set_camera(cam) and Reset() in one call that does not wait for the GPU: the history is
        kept across the move (with moments off or fewer than 2 frames it is set_camera + Reset). The history is
        taken under the camera of the last Render(); `self.camera`, when set, becomes `cam`."""
        d = cam._desc()
        check(lib.rt2_tracer_move_camera(self._h, ctypes.byref(d), _temporal_params(temporal_params)))
        if self.camera is not None:
            self.camera = cam

    def present_time(self) -> float:
        """GPU ms of the last present's kernels (-1: not finished yet, or none). Never waits."""
        return self._ms(lib.rt2_tracer_present_time)

    # -- reconstructing the gathered image (rt2.h "Reconstructing the gathered image") -----------
    # For create_multi, joined and plain tracers; arrays have the shape of the whole image, on rank 0.
    def gather_estimate(self) -> None:
        """gather() with the sums of squares: the root then also holds the variance of the mean (collective on
        joined tracers; enqueued, no wait). Needs enable_moments and FrameIdx() >= 2."""
        self._push_camera()
        check(lib.rt2_tracer_gather_estimate(self._h))

    def image_variance(self) -> np.ndarray:
        """The gathered estimate's variance of the mean, (H, W) float32: denoise()'s input v."""
        w, h = self.Dims()
        out = np.zeros((h, w), np.float32)
        check(lib.rt2_tracer_image_variance(self._h, _fp(out)))
        return out

    def image_features(self) -> np.ndarray:
        """features() of the whole image, (H, W, 16) float32, traced on the root (needs no gather, no moments)."""
        self._push_camera()
        w, h = self.Dims()
        out = np.zeros((h, w, 16), np.float32)
        check(lib.rt2_tracer_image_features(self._h, _fp(out)))
        return out

    def image_resolve(self, variance: bool = False, length: bool = False, **present_params):
        """temporal_resolve() and denoise() in one over the gathered estimate: (H, W, 3) float32; with variance /
        length also the variance of the mean and the blend's length in frames, (H, W) each (length stays zero with
        temporal off). present_params: present()'s (temporal, denoise, tp, dp). Changes nothing."""
        self._push_camera()
        w, h = self.Dims()
        out = np.zeros((h, w, 3), np.float32)
        var = np.zeros((h, w), np.float32) if variance else None
        ln = np.zeros((h, w), np.float32) if length else None
        check(lib.rt2_tracer_image_resolve(self._h, _present_params(present_params), _fp(out),
                                           _fp(var) if variance else None, _fp(ln) if length else None))
        res = (out,) + ((var,) if variance else ()) + ((ln,) if length else ())
        return res if len(res) > 1 else out

    def image_present(self, **params) -> np.ndarray:
        """present() of the gathered image, (H, W, 4) uint8."""
        self._push_camera()
        w, h = self.Dims()
        out = np.zeros((h, w, 4), np.uint8)
        check(lib.rt2_tracer_image_present(self._h, _present_params(params),
                                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def image_present_async(self, pinned_array: np.ndarray, **params) -> None:
        """image_present() enqueued into `pinned_array` ((H, W, 4) uint8 of a progressive.PinnedBuffer), returning
        at once: the bytes are complete after synchronize() or once query() returns 1."""
        w, h = self.Dims()
        a = pinned_array
        if a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"] or a.nbytes != h * w * 4:
            raise ValueError("image_present_async: need a C-contiguous uint8 array of H * W * 4 bytes")
        self._push_camera()
        check(lib.rt2_tracer_image_present_async(self._h, _present_params(params),
                                                 a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def image_move_camera(self, cam: Camera, **temporal_params) -> None:
        """move_camera() for the gathered image: the blend of the current gathered estimate becomes the root's
        history, then set_camera(cam) and Reset() on every GPU, without a wait (collective on joined tracers).
        `self.camera`, when set, becomes `cam`."""
        d = cam._desc()
        check(lib.rt2_tracer_image_move_camera(self._h, ctypes.byref(d), _temporal_params(temporal_params)))
        if self.camera is not None:
            self.camera = cam

    def image_present_time(self) -> float:
        """GPU ms of the last image present's kernels (-1: not finished yet, or none). Never waits."""
        return self._ms(lib.rt2_tracer_image_present_time)

    # -- adaptive sampling of the gathered image (rt2.h "Adaptive sampling of the gathered image") -----
    # adaptive sampling for create_multi and joined tracers (and plain ones): the counts travel with the gather.
    def image_enable_adaptive(self, on: bool = True) -> None:
        """enable_adaptive() on every GPU of the tracer (on a joined tracer: on this rank, after join()); gathers
        then carry each pixel's sample count (needs enable_moments; resets the frame)."""
        check(lib.rt2_tracer_image_enable_adaptive(self._h, 1 if on else 0))

    def image_adaptive_check(self, threshold: float, window: int = 1) -> dict:
        """adaptive_check() on every GPU, the checks overlapping; rt2_adaptive of the whole image as a dict
        (collective on joined tracers: every rank gets the same dict)."""
        a = Adaptive()
        check(lib.rt2_tracer_image_adaptive_check(self._h, float(threshold), int(window), ctypes.byref(a)))
        return a.as_dict()

    def image_render_adaptive(self, threshold: float, max_frames: int, window: int = 1, min_frames: int = 0,
                              check_every: int = 0) -> dict:
        """render_adaptive() over image_adaptive_check(): until the whole image has no active pixel or FrameIdx()
        reaches max_frames; returns the last check."""
        self._push_camera()
        a = Adaptive()
        check(lib.rt2_tracer_image_render_adaptive(self._h, float(threshold), int(window), int(min_frames),
                                                   int(max_frames), int(check_every), ctypes.byref(a)))
        return a.as_dict()

    def image_part_adaptive(self, part: int) -> dict:
        """The last check's rt2_adaptive of GPU `part` alone, before the sum over the GPUs."""
        a = Adaptive()
        check(lib.rt2_tracer_image_part_adaptive(self._h, int(part), ctypes.byref(a)))
        return a.as_dict()

    def image_sample_counts(self) -> np.ndarray:
        """uint32 sample count n_p per pixel of the gathered image, (H, W), on rank 0 (after gather())."""
        w, h = self.Dims()
        out = np.zeros((h, w), np.uint32)
        check(lib.rt2_tracer_image_sample_counts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def enable_stats(self, on: bool = True) -> None:
        check(lib.rt2_tracer_enable_stats(self._h, 1 if on else 0))

    def stats(self) -> dict:
        s = Stats()
        check(lib.rt2_tracer_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def part_stats(self, part: int) -> dict:
        """Stats of GPU `part` of a multi-GPU tracer (rt2_tracer_part_stats)."""
        s = Stats()
        check(lib.rt2_tracer_part_stats(self._h, part, ctypes.byref(s)))
        return s.as_dict()

    def image_non_converted_pixels_async(self, out_ptr: int) -> None:
        """NonConvertedPixels of the gathered image into pinned host memory at out_ptr (rt2_host_alloc,
        height * width * 3 floats), enqueued; complete after synchronize() or query() == 1."""
        check(lib.rt2_tracer_image_non_converted_pixels_async(self._h, ctypes.c_void_p(out_ptr)))

    def reset_stats(self) -> None:
        check(lib.rt2_tracer_reset_stats(self._h))
