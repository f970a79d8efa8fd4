"""Thin Python handle over the C ABI: one Context per HIP device."""
import ctypes

import numpy as np

from . import abi


class Context:
    def __init__(self, device=0):
        self.lib = abi.load()
        h = ctypes.c_void_p()
        st = self.lib.rt_context_create(device, ctypes.byref(h))
        if st != abi.RT_OK:
            raise abi.RTError(st, self.lib.rt_last_error(None).decode())
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.rt_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != abi.RT_OK:
            raise abi.RTError(st, self.lib.rt_last_error(self.h).decode())

    def upload(self, desc):
        self._check(self.lib.rt_scene_upload(self.h, ctypes.byref(desc)))

    def set_timing(self, on):
        self._check(self.lib.rt_set_timing(self.h, 1 if on else 0))

    def stats(self):
        c = abi.rt_counters()
        self._check(self.lib.rt_stats(self.h, ctypes.byref(c)))
        return c

    def reset_counters(self):
        self._check(self.lib.rt_reset_counters(self.h))

    @staticmethod
    def params(spp, max_depth, seed=1, precision=abi.RT_PREC_F32, first_sample=0, samples_per_item=0, pool_slots=0,
               segments_per_launch=0, traversal=0):
        return abi.rt_render_params(spp=spp, max_depth=max_depth, seed=seed, precision=precision,
                                    first_sample=first_sample, samples_per_item=samples_per_item,
                                    pool_slots=pool_slots, segments_per_launch=segments_per_launch,
                                    traversal=traversal)

    def render_tiles(self, cam, params, tiles, out_ptr, out_is_device, stream=None):
        """`tiles`: a list of (x, y, w, h), or an abi.TileList built once for tiles rendered every frame."""
        arr = tiles.arr if isinstance(tiles, abi.TileList) else abi.TileList(tiles).arr
        self._check(self.lib.rt_render_tiles(self.h, ctypes.byref(cam), ctypes.byref(params), arr, len(tiles),
                                             ctypes.c_void_p(out_ptr), int(out_is_device),
                                             ctypes.c_void_p(stream or 0)))

    def render(self, cam, spp, max_depth, seed=1, precision=abi.RT_PREC_F32, tiles=None, **kw):
        """Render to a host numpy array (H, W, 3) -- or the packed tiles, (npix, 3)."""
        p = self.params(spp, max_depth, seed, precision, **kw)
        full = tiles is None
        if full:
            tiles = [(0, 0, cam.image_width, cam.image_height)]
        npix = sum(t[2] * t[3] for t in tiles)
        out = np.zeros((npix, 3), dtype=np.float64 if precision == abi.RT_PREC_F64 else np.float32)
        self.render_tiles(cam, p, tiles, out.ctypes.data, 0)
        return out.reshape(cam.image_height, cam.image_width, 3) if full else out

    def last_kernel(self):
        """The tag of the path kernel the last render on this host thread launched (rt_dev_last_kernel): the
        traversal policy with its template arguments, "camx" for the extended form, and the schedule, e.g.
        "FlatTrav<f64,1,1> persist"; "" before the first render. Per host thread, not per context."""
        buf = ctypes.create_string_buffer(128)
        self.lib.rt_dev_last_kernel(buf, len(buf))
        return buf.value.decode()

    def last_run(self):
        """The run length of the units that kernel's queue handed out (rt_dev_last_run): L where the launch took the
        runs form of a kernel (csrc/rt_plan.h RunPlan), 1 where its units were items, 0 before the first render."""
        return int(self.lib.rt_dev_last_run())

    def trace_family(self, precision=abi.RT_PREC_F64, traversal=0):
        """The traversal trace_rays takes for the uploaded scene: "FLAT", "LINEAR", "WIDE_LDS", "WIDE_HBM", "STACK"."""
        f = self.lib.rt_trace_family(self.h, precision, traversal)
        if f < 0:
            raise abi.RTError(abi.RT_ERR_NO_SCENE if precision in (abi.RT_PREC_F32, abi.RT_PREC_F64) and
                              traversal in (abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED) else abi.RT_ERR_INVALID_ARGUMENT,
                              "no scene uploaded, or an unknown precision or traversal")
        return abi.TRACE_FAMILY_NAMES[f]

    def trace_rays(self, rays, precision=abi.RT_PREC_F64, traversal=0, seed=1, stream=None):
        """Closest hits of `rays`, (n, 8) float64 rows o[3], d[3], time, tmax -> (geom, ids): geom (n, 7) float64
        t, p[3], n[3]; ids (n, 4) int32 object, material, kind, front (a miss: t = inf, ids -1).

        A C-contiguous numpy array takes the host path and returns numpy arrays once they are filled. A float64
        torch tensor on the context's device takes the device path: the call is ordered on `stream` (a
        torch.cuda.Stream or a raw handle; default torch's current stream) and returns tensors on that device."""
        dev, n, src, sp, stream = self._ray_source(rays, stream)
        prm = abi.rt_trace_params(seed=seed, precision=precision, traversal=traversal, on_device=int(dev is not None))
        geom, gp = self._output(n, (7,), "float64", dev)
        ids, ip = self._output(n, (4,), "int32", dev)
        self._check(self.lib.rt_trace_rays(self.h, ctypes.byref(prm), sp, n, gp, ip, stream))
        return geom, ids

    def occluded(self, rays, precision=abi.RT_PREC_F64, traversal=0, seed=1, stream=None, out=None):
        """Whether anything lies on each ray within [0.001, tmax]: `rays` as trace_rays takes them -> (n,) uint8, 1
        exactly where trace_rays with the same arguments reports a hit. An any-hit query with early exit
        (rt_occluded): for a segment from p to q pass o = p, d = q - p and a tmax just below 1.

        A C-contiguous numpy array takes the host path and returns a numpy array; a float64 torch tensor on the
        context's device takes the device path, ordered on `stream` (default torch's current stream), and returns a
        torch.uint8 tensor on that device -- the first n bytes of `out` where one is given (device path only: a
        contiguous torch.uint8 tensor of at least n elements on that device; the call writes nothing past them)."""
        dev, n, src, sp, stream = self._ray_source(rays, stream)
        prm = abi.rt_trace_params(seed=seed, precision=precision, traversal=traversal, on_device=int(dev is not None))
        if out is None:
            out, op = self._output(n, (), "uint8", dev)
        elif dev is None:
            raise ValueError("out: only with the device path")
        else:
            import torch
            if not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.uint8 and
                    out.dim() == 1 and out.is_contiguous() and out.shape[0] >= max(n, 1)):
                raise ValueError("out: a contiguous 1-D torch.uint8 tensor of at least n elements on the rays' device")
            # (the whole tensor's pointer: an empty slice has none, and the call checks its arguments even for n = 0)
            out, op = out[:n], out.data_ptr()
        self._check(self.lib.rt_occluded(self.h, ctypes.byref(prm), sp, n, op, stream))
        return out

    def radiance(self, rays, spp, max_depth, seed=1, precision=abi.RT_PREC_F32, traversal=0, first_sample=0,
                 samples_per_item=0, ray_base=0, stream=None):
        """Path-traced radiance along `rays` (rt_radiance), rows as trace_rays takes them (tmax is not read; a NaN time
        makes every sample draw its own) -> (n, 3) of the precision's dtype: per ray the mean of ray_color over samples
        [first_sample, first_sample + spp), ray i keyed as pixel ray_base + i of a render with this seed.

        A C-contiguous numpy array takes the host path and returns a numpy array; a float64 torch tensor on the
        context's device takes the device path, ordered on `stream` (default torch's current stream), and returns a
        tensor on that device."""
        dev, n, src, sp, stream = self._ray_source(rays, stream)
        prm = abi.rt_radiance_params(seed=seed, spp=spp, first_sample=first_sample, max_depth=max_depth,
                                     precision=precision, traversal=traversal, samples_per_item=samples_per_item,
                                     ray_base=ray_base, on_device=int(dev is not None))
        out, op = self._output(n, (3,), "float64" if precision == abi.RT_PREC_F64 else "float32", dev)
        self._check(self.lib.rt_radiance(self.h, ctypes.byref(prm), sp, n, op, stream))
        return out

    def _ray_source(self, rays, stream):
        """What trace_rays, occluded and radiance make of their `rays` and `stream`: (the rays' torch device, or None for the
        host path; n; the array to read -- one padding row for n = 0: an empty array still hands over a valid pointer,
        since the call checks its arguments and launches nothing -- and its pointer; the stream handle or None)."""
        if isinstance(rays, np.ndarray):
            if rays.dtype != np.float64 or rays.ndim != 2 or rays.shape[1] != 8 or not rays.flags.c_contiguous:
                raise ValueError("rays: a C-contiguous (n, 8) float64 array")
            n = rays.shape[0]
            src = rays if n else np.zeros((1, 8))
            return None, n, src, src.ctypes.data, self._stream_handle(stream) if stream else None
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float64 and rays.dim() == 2 and
                rays.shape[1] == 8 and rays.is_contiguous()):
            raise ValueError("rays: a contiguous (n, 8) float64 numpy array or CUDA/HIP torch tensor")
        n = rays.shape[0]
        src = rays if n else torch.zeros((1, 8), dtype=torch.float64, device=rays.device)
        return rays.device, n, src, src.data_ptr(), self._torch_stream(stream, rays.device)

    @staticmethod
    def _output(n, cols, dtype, dev, fill=None):
        """An output of n rows of shape `cols`: a numpy array (dev None) or a torch tensor on `dev`, uninitialised or
        filled with `fill`, and the pointer to hand over -- of a buffer of at least one row, of which the output is
        the first n, so that the pointer is valid for n = 0 too."""
        shape = (n or 1,) + cols
        if dev is None:
            base = np.empty(shape, dtype) if fill is None else np.full(shape, fill, dtype)
            return (base if n else base[:0]), base.ctypes.data
        import torch
        dt = getattr(torch, dtype)
        base = torch.empty(shape, dtype=dt, device=dev) if fill is None else torch.full(shape, fill, dtype=dt, device=dev)
        return (base if n else base[:0]), base.data_ptr()

    def _torch_stream(self, stream, dev):
        """The handle of `stream`, a torch.cuda.Stream or a raw handle; None: torch's current stream on `dev`."""
        import torch
        return self._stream_handle(torch.cuda.current_stream(dev) if stream is None else stream)

    def _tiles(self, cam, tiles):
        """(ctypes tile array, count, pixels, whether it is the whole image as one tile)."""
        full = tiles is None
        if full:
            tiles = [(0, 0, cam.image_width, cam.image_height)]
        tl = tiles if isinstance(tiles, abi.TileList) else abi.TileList(tiles)
        return tl.arr, len(tl), sum(t[2] * t[3] for t in tl), full

    def camera_rays(self, cam, spp, seed=1, first_sample=0, tiles=None, device=False, stream=None):
        """The camera rays a render draws, (npix * spp, 8) float64 rows o[3], d[3], time, tmax = inf in trace_rays'
        format: row pix * spp + s is sample first_sample + s of pixel pix, pixels packed as render packs its tiles
        (default: the whole image, row-major). Needs no scene. device=False: a numpy array; device=True: a torch
        tensor on the context's device, the call ordered on `stream` (default torch's current stream)."""
        arr, nt, npix, _ = self._tiles(cam, tiles)
        dev, sp = self._output_device(device, stream)
        out, op = self._output(npix * spp, (8,), "float64", dev)
        self._check(self.lib.rt_camera_rays(self.h, ctypes.byref(cam), seed, first_sample, spp, arr, nt,
                                            op, 1 if device else 0, sp))
        return out

    def _output_device(self, device, stream):
        """What camera_rays and render_aov make of `device` and `stream`: (the context's torch device and the stream
        handle, or None twice for host outputs)."""
        if not device:
            return None, None
        import torch
        dev = torch.device("cuda", self.device)
        return dev, self._torch_stream(stream, dev)

    def render_aov(self, cam, spp, seed=1, precision=abi.RT_PREC_F32, traversal=0, first_sample=0, tiles=None,
                   device=False, stream=None):
        """The first-hit feature buffers of the frame, the means over samples [first_sample, first_sample + spp) of
        each pixel: dict(albedo (.., 3), normal (.., 3), depth (..), hit (..), ids (.., 4) int32 object, material,
        kind, front of sample first_sample). Shapes are (H, W, ..) for the whole image, (npix, ..) for given tiles.
        float64 for both precisions. device=False: numpy arrays, filled on return; device=True: torch tensors (views
        of one buffer) on the context's device, the call ordered on `stream` (default torch's current stream)."""
        arr, nt, npix, full = self._tiles(cam, tiles)
        prm = abi.rt_aov_params(seed=seed, spp=spp, first_sample=first_sample, precision=precision,
                                traversal=traversal, on_device=1 if device else 0)
        dev, sp = self._output_device(device, stream)
        feat, fp = self._output(npix, (8,), "float64", dev, fill=0.0)
        ids, ip = self._output(npix, (4,), "int32", dev, fill=-1)
        self._check(self.lib.rt_render_aov(self.h, ctypes.byref(cam), ctypes.byref(prm), arr, nt, fp, ip, sp))
        shape = (cam.image_height, cam.image_width) if full else (npix,)
        return dict(albedo=feat[:, 0:3].reshape(*shape, 3), normal=feat[:, 3:6].reshape(*shape, 3),
                    depth=feat[:, 6].reshape(*shape), hit=feat[:, 7].reshape(*shape), ids=ids.reshape(*shape, 4))

    def render_adaptive(self, cam, max_spp, max_depth, threshold, min_spp=None, step_spp=None, batch=4, floor=0.01,
                        seed=1, precision=abi.RT_PREC_F32, traversal=0, tiles=None, device=False, stream=None):
        """An adaptively sampled frame with its noise map (rt_render_adaptive): dict(rgb (.., 3) of the precision's
        dtype, spp (..) int32 the samples each pixel took, err (..) float64 its final error estimate). Every pixel takes
        min_spp samples, then step_spp more per round until its estimated relative standard error is <= threshold or it
        has max_spp; the estimate is the batch-means one over batches of `batch` samples (include/rt_hip.h). Defaults:
        step_spp = 4 * batch, min_spp = step_spp. Shapes are (H, W, ..) for the whole image, (npix, ..) for given
        tiles. device=False: numpy arrays, filled on return; device=True: torch tensors on the context's device, the
        call ordered on `stream` (default torch's current stream)."""
        step_spp = 4 * batch if step_spp is None else step_spp
        min_spp = step_spp if min_spp is None else min_spp
        arr, nt, npix, full = self._tiles(cam, tiles)
        prm = abi.rt_adaptive_params(seed=seed, min_spp=min_spp, max_spp=max_spp, step_spp=step_spp, batch=batch,
                                     max_depth=max_depth, precision=precision, traversal=traversal,
                                     on_device=1 if device else 0, threshold=threshold, floor=floor)
        dev, sp = self._output_device(device, stream)
        rgb, rp = self._output(npix, (3,), "float64" if precision == abi.RT_PREC_F64 else "float32", dev, fill=0.0)
        spp, np_ = self._output(npix, (), "int32", dev, fill=0)
        err, ep = self._output(npix, (), "float64", dev, fill=0.0)
        self._check(self.lib.rt_render_adaptive(self.h, ctypes.byref(cam), ctypes.byref(prm), arr, nt, rp, np_, ep, sp))
        shape = (cam.image_height, cam.image_width) if full else (npix,)
        return dict(rgb=rgb.reshape(*shape, 3), spp=spp.reshape(*shape), err=err.reshape(*shape))

    def denoise(self, rgb, aov, var=None, iterations=5, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0,
                demodulate=True, albedo_eps=1e-2, color_eps=1e-8, depth_eps=1e-3, stream=None):
        """The frame `rgb`, (H, W, 3) float32 or float64, filtered by the variance-guided a-trous filter (rt_denoise):
        spatial, single-frame, guided by `aov` -- render_aov's dict, or its rows as an (H, W, 8) or (npix, 8) float64
        array albedo[3], normal[3], depth, hit -- and by `var`, (H, W) float64, the summed variance of the three channel
        means (adaptive_variance of render_adaptive's dict; None: sigma_color is an absolute colour distance). The
        precision is rgb's dtype. Needs no scene. -> (H, W, 3) of rgb's kind and dtype.

        numpy inputs take the host path; torch tensors on the context's device take the device path, ordered on
        `stream` (default torch's current stream). The three inputs are of one kind."""
        dev = None if isinstance(rgb, np.ndarray) else rgb.device
        if dev is None:
            xp, f64, f32, cat = np, np.float64, np.float32, np.concatenate
            contiguous, ptr = np.ascontiguousarray, (lambda a: a.ctypes.data)
        else:
            import torch
            if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda):
                raise ValueError("rgb: a numpy array or a CUDA/HIP torch tensor")
            xp, f64, f32, cat = torch, torch.float64, torch.float32, torch.cat
            contiguous, ptr = (lambda a: a.contiguous()), (lambda a: a.data_ptr())
        if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype not in (f32, f64):
            raise ValueError("rgb: an (H, W, 3) float32 or float64 array or tensor")
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        if isinstance(aov, dict):
            aov = cat([aov["albedo"].reshape(H * W, 3), aov["normal"].reshape(H * W, 3),
                       aov["depth"].reshape(H * W, 1), aov["hit"].reshape(H * W, 1)], 1)
        if not isinstance(aov, type(rgb)) or aov.dtype != f64 or aov.shape[-1] != 8 or int(np.prod(aov.shape)) != H * W * 8:
            raise ValueError("aov: render_aov's dict, or an (H, W, 8) or (npix, 8) float64 array of rgb's kind")
        if var is not None and (not isinstance(var, type(rgb)) or var.dtype != f64 or int(np.prod(var.shape)) != H * W):
            raise ValueError("var: an (H, W) float64 array of rgb's kind")
        if dev is not None and any(t is not None and t.device != dev for t in (aov, var)):
            raise ValueError("rgb, aov and var must be on one device")
        rgb, aov = contiguous(rgb), contiguous(aov)
        var = None if var is None else contiguous(var)
        prm = abi.rt_denoise_params(width=W, height=H, iterations=iterations,
                                    precision=abi.RT_PREC_F64 if rgb.dtype == f64 else abi.RT_PREC_F32,
                                    on_device=int(dev is not None), flags=abi.RT_DENOISE_DEMODULATE if demodulate else 0,
                                    sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_depth=sigma_depth,
                                    albedo_eps=albedo_eps, color_eps=color_eps, depth_eps=depth_eps)
        out = xp.empty_like(rgb)
        sp = None if dev is None else self._torch_stream(stream, dev)
        self._check(self.lib.rt_denoise(self.h, ctypes.byref(prm), ptr(rgb), ptr(aov),
                                        None if var is None else ptr(var), ptr(out), sp))
        return out

    def temporal(self, cam, prev_cam, rgb, aov, var=None, ids=None, hist=None, alpha_min=0.05, max_history=64,
                 depth_tol=0.05, normal_cos=0.9, min_weight=0.25, demodulate=True, albedo_eps=1e-2, stream=None,
                 hist_out=None):
        """The frame `rgb`, (H, W, 3) float32 or float64, blended with the accumulated frames before it (rt_temporal):
        `hist`, the "hist" of the call before (None: a first frame), is reprojected from `prev_cam` into `cam` through
        this frame's guides `aov` (as Context.denoise takes them), history that no longer shows the same surface is
        rejected, and the rest is blended with weight max(alpha_min, 1 / (N + 1)). `var`: (H, W) float64 as for denoise,
        or None; `ids`: render_aov's "ids", (H, W, 4) int32, or None. The precision is rgb's dtype. Needs no scene.
        -> dict(rgb (H, W, 3), var (H, W) float64 -- what denoise takes as var --, hist, a uint8 buffer of
        rt_temporal_history_bytes bytes to hand to the next call, count (H, W), a view of hist's N plane).

        `hist_out`: a buffer of hist's kind and size to write the new history into (not `hist` itself: the call reads
        one while it writes the other), for a caller that keeps two and swaps them; None: a new one.
        With a still camera pass normal_cos = -1 (progressive rendering): a guide normal is a mean over the pixel's
        samples, shorter than 1 where the pixel straddles an edge, and the default 0.9 drops such a pixel's history.

        numpy inputs take the host path; torch tensors on the context's device take the device path, ordered on
        `stream` (default torch's current stream). All arrays are of one kind."""
        dev = None if isinstance(rgb, np.ndarray) else rgb.device
        if dev is not None:
            import torch
            if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.device.index == self.device):
                raise ValueError("rgb: a numpy array or a torch tensor on the context's device")
        prm, rgb, aov, var, ids, hist, ptr = _temporal_inputs(rgb, aov, var, ids, hist, int(dev is not None), alpha_min,
                                                              max_history, depth_tol, normal_cos, min_weight,
                                                              demodulate, albedo_eps)
        H, W = prm.height, prm.width
        if hist_out is not None and not (isinstance(hist_out, type(rgb)) and hist_out.dtype == (np if dev is None else torch).uint8 and
                                         hist_out.ndim == 1 and int(hist_out.shape[0]) == _history_bytes(prm) and
                                         (dev is None or hist_out.device == dev) and
                                         (hist_out.flags.c_contiguous if dev is None else hist_out.is_contiguous())):
            raise ValueError("hist_out: a contiguous uint8 buffer of hist's kind and size")
        if dev is None:
            out, var_out = np.empty_like(rgb), np.empty((H, W), np.float64)
            hist_out = np.empty(_history_bytes(prm), np.uint8) if hist_out is None else hist_out
        else:
            out, var_out = torch.empty_like(rgb), torch.empty((H, W), dtype=torch.float64, device=dev)
            hist_out = torch.empty(_history_bytes(prm), dtype=torch.uint8, device=dev) if hist_out is None else hist_out
        sp = None if dev is None else self._torch_stream(stream, dev)
        self._check(self.lib.rt_temporal(self.h, ctypes.byref(prm), ctypes.byref(cam),
                                         None if prev_cam is None else ctypes.byref(prev_cam), ptr(rgb), ptr(aov),
                                         ptr(ids), ptr(var), ptr(hist), ptr(hist_out), ptr(out), ptr(var_out), sp))
        return dict(rgb=out, var=var_out, hist=hist_out, count=history_planes(hist_out, W, H, rgb.dtype)["count"])

    @staticmethod
    def _stream_handle(stream):
        return int(getattr(stream, "cuda_stream", stream) or 0)


class Multi:
    """rt_multi_*: one process driving several devices (tiles round-robin, RCCL gather to devices[0])."""

    def __init__(self, devices):
        self.lib = abi.load()
        arr = (ctypes.c_int32 * len(devices))(*devices)
        h = ctypes.c_void_p()
        st = self.lib.rt_multi_create(arr, len(devices), ctypes.byref(h))
        if st != abi.RT_OK:
            raise abi.RTError(st, self.lib.rt_multi_last_error(None).decode())
        self.h, self.n = h, len(devices)

    def close(self):
        if self.h:
            self.lib.rt_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != abi.RT_OK:
            raise abi.RTError(st, self.lib.rt_multi_last_error(self.h).decode())

    @property
    def uses_rccl(self):
        return bool(self.lib.rt_multi_uses_rccl(self.h))

    def upload(self, desc):
        self._check(self.lib.rt_multi_scene_upload(self.h, ctypes.byref(desc)))

    def render(self, cam, spp, max_depth, seed=1, precision=abi.RT_PREC_F32, tile_size=0, **kw):
        p = Context.params(spp, max_depth, seed, precision, **kw)
        out = np.zeros((cam.image_height, cam.image_width, 3),
                       dtype=np.float64 if precision == abi.RT_PREC_F64 else np.float32)
        self._check(self.lib.rt_multi_render(self.h, ctypes.byref(cam), ctypes.byref(p), tile_size, out.ctypes.data))
        return out

    def stats(self, rank):
        c = abi.rt_counters()
        self._check(self.lib.rt_multi_stats(self.h, rank, ctypes.byref(c)))
        return c


def adaptive_variance(out, floor=0.01):
    """render_adaptive's dict (with the `floor` it was rendered with) -> the `var` Context.denoise takes: per pixel the
    summed variance of the three channel means, (err * (floor + level))^2 * 3 with level the mean of the pixel's
    channels (the estimator's se2, include/rt_hip.h), float64, numpy or torch as the dict's arrays are."""
    rgb, err = out["rgb"], out["err"]
    if isinstance(rgb, np.ndarray):
        level = rgb.astype(np.float64).sum(-1) / 3.0
    else:
        level = rgb.double().sum(-1) / 3.0
    return (err * (floor + level)) ** 2 * 3.0


def denoise_host(rgb, feat, var=None, iterations=5, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0,
                 demodulate=True, albedo_eps=1e-2, color_eps=1e-8, depth_eps=1e-3):
    """Context.denoise's passes run by a host loop over the kernels' own arithmetic (rt_dev_denoise_host): numpy
    arrays, rgb (H, W, 3) float32 or float64, feat (H * W, 8) float64, var (H, W) float64 or None. No GPU, no Context;
    a development helper for tests."""
    H, W = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb)
    feat = np.ascontiguousarray(feat, np.float64)
    var = None if var is None else np.ascontiguousarray(var, np.float64)
    prm = abi.rt_denoise_params(width=W, height=H, iterations=iterations,
                                precision=abi.RT_PREC_F64 if rgb.dtype == np.float64 else abi.RT_PREC_F32, on_device=0,
                                flags=abi.RT_DENOISE_DEMODULATE if demodulate else 0, sigma_color=sigma_color,
                                sigma_normal=sigma_normal, sigma_depth=sigma_depth, albedo_eps=albedo_eps,
                                color_eps=color_eps, depth_eps=depth_eps)
    out = np.empty_like(rgb)
    st = abi.load().rt_dev_denoise_host(ctypes.byref(prm), rgb.ctypes.data, feat.ctypes.data,
                                        None if var is None else var.ctypes.data, out.ctypes.data)
    if st != abi.RT_OK:
        raise abi.RTError(st, "rt_dev_denoise_host: parameters rt_denoise_check refuses")
    return out


def _history_bytes(prm):
    return int(abi.load().rt_temporal_history_bytes(prm.width, prm.height, prm.precision))


def _temporal_inputs(rgb, aov, var, ids, hist, on_device, alpha_min, max_history, depth_tol, normal_cos, min_weight,
                     demodulate, albedo_eps):
    """What Context.temporal and temporal_host make of their arrays: (the parameters, the five arrays contiguous and
    checked -- aov as (npix, 8) rows --, the function that gives an array's pointer, None for None)."""
    if isinstance(rgb, np.ndarray):
        f64, f32, i32, u8, cat, contiguous = np.float64, np.float32, np.int32, np.uint8, np.concatenate, np.ascontiguousarray
        ptr = lambda a: None if a is None else a.ctypes.data
    else:
        import torch
        f64, f32, i32, u8, cat = torch.float64, torch.float32, torch.int32, torch.uint8, torch.cat
        contiguous = lambda a: a.contiguous()
        ptr = lambda a: None if a is None else a.data_ptr()
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype not in (f32, f64):
        raise ValueError("rgb: an (H, W, 3) float32 or float64 array or tensor")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if isinstance(aov, dict):
        aov = cat([aov["albedo"].reshape(H * W, 3), aov["normal"].reshape(H * W, 3),
                   aov["depth"].reshape(H * W, 1), aov["hit"].reshape(H * W, 1)], 1)
    same = lambda a: isinstance(a, type(rgb)) and (isinstance(a, np.ndarray) or a.device == rgb.device)
    if not same(aov) or aov.dtype != f64 or aov.shape[-1] != 8 or int(np.prod(aov.shape)) != H * W * 8:
        raise ValueError("aov: render_aov's dict, or an (H, W, 8) or (npix, 8) float64 array of rgb's kind")
    if var is not None and (not same(var) or var.dtype != f64 or int(np.prod(var.shape)) != H * W):
        raise ValueError("var: an (H, W) float64 array of rgb's kind")
    if ids is not None and (not same(ids) or ids.dtype != i32 or ids.shape[-1] != 4 or int(np.prod(ids.shape)) != H * W * 4):
        raise ValueError("ids: an (H, W, 4) int32 array of rgb's kind")
    prm = abi.rt_temporal_params(width=W, height=H, precision=abi.RT_PREC_F64 if rgb.dtype == f64 else abi.RT_PREC_F32,
                                 on_device=on_device, flags=abi.RT_TEMPORAL_DEMODULATE if demodulate else 0,
                                 max_history=max_history, alpha_min=alpha_min, depth_tol=depth_tol,
                                 normal_cos=normal_cos, min_weight=min_weight, albedo_eps=albedo_eps)
    if hist is not None and (not same(hist) or hist.dtype != u8 or hist.ndim != 1 or
                             int(hist.shape[0]) != _history_bytes(prm)):
        raise ValueError("hist: the hist of a call on a frame of this size and dtype")
    opt = lambda a: None if a is None else contiguous(a)
    return prm, contiguous(rgb), contiguous(aov), opt(var), opt(ids), opt(hist), ptr


def history_planes(hist, W, H, dtype):
    """Views of the four planes of a history buffer (include/rt_hip.h, "temporal accumulation"), a 1-D uint8 numpy
    array or torch tensor: dict(color (H, W, 4) {c.r, c.g, c.b, v}, guide (H, W, 4) {n.x, n.y, n.z, z}, count (H, W),
    id (H, W) int32), the first three of `dtype` (rgb's)."""
    if isinstance(hist, np.ndarray):
        size, i32 = np.dtype(dtype).itemsize, np.int32
    else:
        import torch
        size, i32 = torch.empty((), dtype=dtype).element_size(), torch.int32
    n = W * H
    plane = lambda lo, hi, dt, *shape: hist[lo:hi].view(dt).reshape(*shape)
    return dict(color=plane(0, 4 * size * n, dtype, H, W, 4), guide=plane(4 * size * n, 8 * size * n, dtype, H, W, 4),
                count=plane(8 * size * n, 9 * size * n, dtype, H, W),
                id=plane(9 * size * n, 9 * size * n + 4 * n, i32, H, W))


def temporal_host(cam, prev_cam, rgb, feat, var=None, ids=None, hist=None, alpha_min=0.05, max_history=64,
                  depth_tol=0.05, normal_cos=0.9, min_weight=0.25, demodulate=True, albedo_eps=1e-2):
    """Context.temporal run by a host loop over the kernel's own arithmetic (rt_dev_temporal_host): numpy arrays, the
    same dict back. No GPU, no Context; a development helper for tests."""
    prm, rgb, feat, var, ids, hist, ptr = _temporal_inputs(rgb, feat, var, ids, hist, 0, alpha_min, max_history,
                                                           depth_tol, normal_cos, min_weight, demodulate, albedo_eps)
    H, W = prm.height, prm.width
    out, var_out = np.empty_like(rgb), np.empty((H, W), np.float64)
    hist_out = np.empty(_history_bytes(prm), np.uint8)
    st = abi.load().rt_dev_temporal_host(ctypes.byref(prm), ctypes.byref(cam),
                                         None if prev_cam is None else ctypes.byref(prev_cam), ptr(rgb), ptr(feat),
                                         ptr(ids), ptr(var), ptr(hist), ptr(hist_out), ptr(out), ptr(var_out))
    if st != abi.RT_OK:
        raise abi.RTError(st, "rt_dev_temporal_host: arguments rt_temporal refuses")
    return dict(rgb=out, var=var_out, hist=hist_out, count=history_planes(hist_out, W, H, rgb.dtype)["count"])


class TemporalAccumulator:
    """Context.temporal over a sequence of frames: keeps the camera of the frame before and two history buffers that
    ping-pong, so a caller's loop is one line per frame. `params`: Context.temporal's keyword parameters. For
    progressive rendering (a still camera, samples split over calls with first_sample) pass alpha_min=0 and
    normal_cos=-1: with the default normal_cos the pixels that straddle an edge keep no history (Context.temporal).

        acc = rt_amd.TemporalAccumulator(ctx, alpha_min=0.1)
        for cam in path:
            out = acc.push(cam, frame(cam)["rgb"], aov(cam), var)   # -> Context.temporal's dict
    """

    def __init__(self, ctx, **params):
        self.ctx, self.params = ctx, params
        self.reset()

    def reset(self):
        """Forget the history: the next frame is a first frame."""
        self.prev_cam, self.hist, self.frames, self._bufs = None, None, 0, [None, None]

    def push(self, cam, rgb, aov, var=None, stream=None):
        """`aov`: render_aov's dict (its "ids" are used) or its rows (no ids). The returned dict's "hist" and "count"
        are views of one of the two buffers: they hold this frame's history until the push after the next one
        overwrites them. Frames of another size, dtype or kind than the one before start again with new buffers."""
        ids = aov.get("ids") if isinstance(aov, dict) else None
        target = self._bufs[self.frames & 1]
        fits = lambda b: (b is not None and isinstance(b, type(rgb)) and
                          (isinstance(b, np.ndarray) or b.device == rgb.device) and int(b.shape[0]) == nbytes)
        nbytes = int(abi.load().rt_temporal_history_bytes(
            int(rgb.shape[1]), int(rgb.shape[0]), abi.RT_PREC_F64 if rgb.dtype.itemsize == 8 else abi.RT_PREC_F32))
        if self.hist is not None and not fits(self.hist):
            self.reset()
            target = None
        out = self.ctx.temporal(cam, self.prev_cam, rgb, aov, var=var, ids=ids, hist=self.hist, stream=stream,
                                hist_out=target if fits(target) else None, **self.params)
        keep = abi.rt_camera_desc()
        ctypes.memmove(ctypes.byref(keep), ctypes.byref(cam), ctypes.sizeof(keep))  # (the caller may move `cam` on)
        self._bufs[self.frames & 1] = out["hist"]
        self.prev_cam, self.hist, self.frames = keep, out["hist"], self.frames + 1
        return out


def multi_plan(w, h, ndev, rank, tile_size=0):
    """rt_multi_plan: the tiles rank `rank` renders (host only)."""
    L = abi.load()
    n = L.rt_multi_plan(w, h, ndev, tile_size, rank, None, 0)
    if n < 0:
        raise ValueError("invalid plan arguments")
    arr = (abi.rt_tile * max(1, n))()
    L.rt_multi_plan(w, h, ndev, tile_size, rank, arr, n)
    return [(t.x0, t.y0, t.width, t.height) for t in arr[:n]]


def plan_kernel(desc, cam, precision=abi.RT_PREC_F32, traversal=0, segments_per_launch=0):
    """The tag of the path kernel Context.render of scene `desc` through camera `cam` with these arguments would launch
    (rt_dev_plan_kernel), in Context.last_kernel's format. The descriptor is compiled on the host: no GPU, no Context."""
    buf = ctypes.create_string_buffer(128)
    abi.load().rt_dev_plan_kernel(ctypes.byref(desc), cam.mode, precision, traversal, segments_per_launch, buf, len(buf))
    if not buf.value:
        raise ValueError("the descriptor does not compile, or an unknown precision or traversal")
    return buf.value.decode()


def plan_radiance_kernel(desc, precision=abi.RT_PREC_F32, traversal=0):
    """The tag of the path kernel Context.radiance on scene `desc` would launch (rt_dev_plan_radiance): plan_kernel's
    for a perspective render on the persistent schedule, with "rays" before the schedule. No GPU, no Context."""
    buf = ctypes.create_string_buffer(128)
    abi.load().rt_dev_plan_radiance(ctypes.byref(desc), precision, traversal, buf, len(buf))
    if not buf.value:
        raise ValueError("the descriptor does not compile, or an unknown precision or traversal")
    return buf.value.decode()
