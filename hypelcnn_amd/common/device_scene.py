"""Scene preparation on the compute device (csrc/scene.hip): the raster file's samples are uploaded as they are and
everything BasicDataSet.__init__ does to them -- symmetric padding, per-band extrema, offset, division, float32 --
plus AVON's per-band percentile clip and the lit/shadow band sums happens where the patch gather will read the result.

`DeviceBasicDataSet` is a BasicDataSet whose scene lives in `casi_dev` / `lidar_dev` (torch tensors on the backend's
device); `.casi` / `.lidar` download it on first use for the host-side consumers (InMemoryImporter, get_data_point,
the host samplers -- gan_sampling_methods.get_sample_pairs_device pairs on the device instead)."""
import numpy
import torch

from hypelcnn_amd.backend import OUT_DTYPES, SCENE_RANK_WS_WORDS, Ref
from hypelcnn_amd.common.common_nn_ops import BasicDataSet, get_data_point_func, get_data_point_func_hsi
from hypelcnn_amd.common.tiff_io import DeviceRaster

EXTREMA_SLICES = 1024  # partial results of a reduction launch (workspace rows)
SUM_SLICES = 2048


def resolve_scene_backend(backend=None):
    """The backend a loader prepares its scene on: the one given, else a HipBackend when a HIP device is visible,
    else None -- the host BasicDataSet."""
    if backend is not None:
        return backend
    if torch.cuda.is_available():
        from hypelcnn_amd.backend import HipBackend
        return HipBackend()
    return None


def make_basic_data_set(backend, **kwargs):
    """BasicDataSet(**kwargs) on the host, DeviceBasicDataSet(**kwargs) when there is a backend."""
    backend = resolve_scene_backend(backend)
    if backend is None:
        clip = kwargs.pop("clip_percentile", None)
        if clip is not None:
            # a copy that keeps the view's memory order, as the reference's astype() does: the float32 band means of
            # the shadow ratio are summed in memory order
            casi = numpy.array(kwargs["casi"], copy=True, order="K")
            bound = numpy.percentile(casi, clip, axis=[0, 1]).astype(casi.dtype)
            numpy.clip(casi, None, bound, out=casi)
            kwargs["casi"] = casi
            data_set = BasicDataSet(**kwargs)
            data_set.clip_bounds = bound
            return data_set
        return BasicDataSet(**kwargs)
    return DeviceBasicDataSet(backend=backend, **kwargs)


def percentile_ranks(n, q):
    """The two ranks numpy.percentile(method="linear") interpolates between, and the weight of the upper one."""
    virtual = (n - 1) * numpy.true_divide(q, 100)
    lo = int(numpy.floor(virtual))
    hi = min(lo + 1, n - 1)
    return lo, hi, virtual - lo


def percentile_from_ranks(a, b, t, dtype):
    """numpy's linear rule in float64 -- a + (b - a) * t, or b - (b - a) * (1 - t) for t >= 0.5 -- then the cast."""
    a, b = numpy.asarray(a), numpy.asarray(b)
    diff = numpy.subtract(b, a)
    out = numpy.asarray(numpy.add(a, diff * t), dtype=numpy.float64)
    if t >= 0.5:
        out = numpy.subtract(b, diff * (1 - t), dtype=numpy.float64)
    return out.astype(dtype)


def resident_view(a, dtype, root_limit=None):
    """What to upload so that the kernels read the NumPy view `a`, as `dtype`, in place: -> (root, element offset of
    a's first item in root, element strides with 0 for an axis of extent 1).  root is the array at the end of a's
    .base chain where that one is C-contiguous, of this dtype and (root_limit) has fewer items than that, and a's
    strides are positive multiples of the item size; else a contiguous copy of a."""
    dtype = numpy.dtype(dtype)
    if a.dtype != dtype:
        a = a.astype(dtype)
    root = a
    while isinstance(root.base, numpy.ndarray):
        root = root.base
    item = dtype.itemsize
    in_place = (root.flags.c_contiguous and root.dtype == dtype and (root_limit is None or root.size < root_limit)
                and all(n == 1 or (s > 0 and s % item == 0) for n, s in zip(a.shape, a.strides)))
    if not in_place:
        root = a = numpy.ascontiguousarray(a)
    offset = (a.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // item
    return root, offset, tuple(0 if n == 1 else int(s) // item for n, s in zip(a.shape, a.strides))


class _Source:
    """A raster in device memory, as the kernels address it: flat byte tensor, element offset, (h, w, bands) and
    element strides.  A view whose root array is contiguous is uploaded as that root and read in place; a
    tiff_io.DeviceRaster is where it is already and is read through its strides, without a copy."""

    def __init__(self, backend, array):
        if isinstance(array, DeviceRaster):
            if array.ndim != 3 or array.dtype not in OUT_DTYPES or 0 in array.shape:
                raise ValueError("scene rasters are [h, w, bands] of float32, uint16, int16 or uint8")
            if array.bytes.device.type != torch.device(backend.device).type:
                raise ValueError("the raster lives on another device than the backend")
            self.dtype = array.dtype
            self.code = OUT_DTYPES[array.dtype]
            self.h, self.w, self.bands = array.shape
            self.strides = tuple(0 if n == 1 else s for n, s in zip(array.shape, array.strides))
            self.bytes = array.bytes
            self.ref = Ref(array.bytes, array.byte_offset)
            return
        a = numpy.asarray(array)
        if a.ndim != 3 or a.dtype not in OUT_DTYPES:
            raise ValueError("scene rasters are [h, w, bands] of float32, uint16, int16 or uint8")
        root, offset, self.strides = resident_view(a, a.dtype)
        self.dtype = a.dtype
        self.code = OUT_DTYPES[a.dtype]
        self.h, self.w, self.bands = (int(v) for v in a.shape)
        self.bytes = torch.from_numpy(root.reshape(-1).view(numpy.uint8)).to(backend.device)
        self.ref = Ref(self.bytes, offset * a.dtype.itemsize)

    def geometry(self):
        return (self.h, self.w, self.bands) + self.strides


class DeviceBasicDataSet(BasicDataSet):
    """BasicDataSet (reference common_nn_ops.py:45-106) prepared by HIP launches.  `clip_percentile`: clip every band
    of the uint16 `casi` at that percentile of the band over the scene first (AVONDataLoader.load_data)."""

    def __init__(self, shadow_creator_dict, casi, lidar, neighborhood, normalize, casi_min=None, casi_max=None,
                 lidar_min=None, lidar_max=None, backend=None, clip_percentile=None):
        if backend is None:
            raise ValueError("DeviceBasicDataSet needs a backend (there is no host fallback: use BasicDataSet)")
        self.backend = backend
        self.neighborhood = neighborhood
        self.shadow_creator_dict = shadow_creator_dict
        self.casi_unnormalized_dtype = casi.dtype
        self.casi_min, self.casi_max, self.lidar_min, self.lidar_max = 0, 1, 0, 1
        self.clip_bounds = None
        self._host = {}
        self._normalized = bool(normalize)
        self.lidar_dev = self.casi_dev = None
        self._dtypes = {}
        if lidar is not None:
            src = _Source(backend, lidar)
            self._dtypes["lidar"] = src.dtype
            lo = scale = None
            if normalize:
                lo, top = self._offset_and_top(src, None, lidar_min, lidar_max)
                self.lidar_min = lo[0] if lidar_min is None else lidar_min
                self.lidar_max = top[0] if lidar_max is None else lidar_max
                scale = numpy.asarray(top).astype(numpy.float32)
            self.lidar_dev = self._prepare(src, None, lo, scale)
        if casi is not None:
            src = _Source(backend, casi)
            self._dtypes["casi"] = src.dtype
            clip = None
            if clip_percentile is not None:
                clip = self.clip_bounds = self._percentile(src, clip_percentile)
            lo = scale = None
            if normalize:
                lo, top = self._offset_and_top(src, clip, casi_min, casi_max)
                self.casi_min = lo if casi_min is None else casi_min
                self.casi_max = top if casi_max is None else casi_max
                scale = numpy.asarray(top).astype(numpy.float32)
            self.casi_dev = self._prepare(src, clip, lo, scale)
        self._get_data_point_func = get_data_point_func if lidar is not None else get_data_point_func_hsi

    # -- launches --
    def _dev(self, array):
        return None if array is None else self.backend.upload(numpy.ascontiguousarray(array).reshape(-1).view(numpy.uint8))

    def _extrema(self, src, clip, sub):
        be = self.backend
        item = src.dtype.itemsize
        out = be.zeros(2 * src.bands * item, torch.uint8)
        ws = be.empty(2 * EXTREMA_SLICES * src.bands * item, torch.uint8)
        clip_d, sub_d = self._dev(clip), self._dev(sub)
        be.call("scene_extrema", src.ref, src.code, *src.geometry(), None if clip_d is None else Ref(clip_d),
                None if sub_d is None else Ref(sub_d), Ref(out), Ref(out, src.bands * item), Ref(ws), EXTREMA_SLICES)
        both = out.cpu().numpy().view(src.dtype)
        return both[:src.bands].copy(), both[src.bands:].copy()

    def _as_source_dtype(self, value, src, what):
        arr = numpy.broadcast_to(numpy.asarray(value), (src.bands,))
        cast = arr.astype(src.dtype)
        if not numpy.array_equal(cast, arr):
            raise ValueError(f"DeviceBasicDataSet: {what} override is not representable in the raster's {src.dtype}")
        return numpy.ascontiguousarray(cast)

    def _offset_and_top(self, src, clip, lo_override, top_override):
        """What BasicDataSet calls *_min and *_max: the per-band minimum, then the maximum of (samples - minimum)
        in the raster's dtype; an override replaces either."""
        lo = None if lo_override is None else self._as_source_dtype(lo_override, src, "minimum")
        raw_max = None
        if lo is None:
            lo, raw_max = self._extrema(src, clip, None)
        if top_override is not None:
            top = numpy.broadcast_to(numpy.asarray(top_override), (src.bands,))
        elif raw_max is not None:
            top = (raw_max - lo).astype(src.dtype)  # max(v - min) = max(v) - min: the rounding is monotone, no wrap
        else:
            top = self._extrema(src, clip, lo)[1]
        return lo, top

    def _percentile(self, src, q):
        if src.dtype != numpy.uint16:
            raise ValueError("the percentile clip is defined for uint16 rasters")
        be = self.backend
        n = src.h * src.w
        lo, hi, t = percentile_ranks(n, q)
        out = be.zeros(2 * src.bands * 2, torch.uint8)
        ws = be.empty(src.bands * SCENE_RANK_WS_WORDS * 4, torch.uint8)
        be.call("scene_rank_select_u16", src.ref, *src.geometry(), lo, hi, Ref(out), Ref(out, src.bands * 2), Ref(ws))
        both = out.cpu().numpy().view(numpy.uint16)
        return percentile_from_ranks(both[:src.bands], both[src.bands:], t, numpy.uint16)

    def _prepare(self, src, clip, lo, scale):
        be = self.backend
        n = int(self.neighborhood)
        out = be.empty((src.h + 2 * n) * (src.w + 2 * n) * src.bands, torch.float32)
        clip_d, lo_d = self._dev(clip), self._dev(lo)
        scale_d = None if scale is None else be.upload(
            numpy.ascontiguousarray(numpy.broadcast_to(scale, (src.bands,)), dtype=numpy.float32))
        be.call("scene_prepare_f32", src.ref, src.code, *src.geometry(), n, None if clip_d is None else Ref(clip_d),
                None if lo_d is None else Ref(lo_d), None if scale_d is None else Ref(scale_d), Ref(out))
        be.synchronize()  # the operands above are released when this returns
        return out.reshape(src.h + 2 * n, src.w + 2 * n, src.bands)

    def masked_band_sums(self, shadow_map):
        """fp64 sums of every band of the prepared casi over shadow_map != 0 and over shadow_map == 0, and the two
        pixel counts: ([2, bands] float64, [2] int64)."""
        be = self.backend
        hp, wp, bands = (int(v) for v in self.casi_dev.shape)
        smap = numpy.asarray(shadow_map)
        if smap.shape != (hp, wp):
            raise ValueError(f"shadow map {smap.shape} does not match the padded scene {(hp, wp)}")
        map_d = be.upload((smap != 0).astype(numpy.uint8))
        out = be.zeros((2 * bands + 2) * 8, torch.uint8)
        ws = be.empty(SUM_SLICES * 2 * (bands + 1) * 8, torch.uint8)
        be.call("scene_masked_sums", Ref(self.casi_dev.reshape(-1)), Ref(map_d), hp, wp, bands, Ref(out),
                Ref(out, 2 * bands * 8), Ref(ws), SUM_SLICES)
        raw = out.cpu().numpy()
        return raw[:2 * bands * 8].view(numpy.float64).reshape(2, bands).copy(), raw[2 * bands * 8:].view(numpy.int64).copy()

    # -- host views --
    def _download(self, name):
        if name not in self._host:
            dev = getattr(self, name + "_dev")
            arr = None
            if dev is not None:
                arr = dev.cpu().numpy()
                if not self._normalized:
                    arr = arr.astype(self._dtypes[name])  # BasicDataSet keeps the raster's dtype then
            self._host[name] = arr
        return self._host[name]

    @property
    def casi(self):
        return self._download("casi")

    @property
    def lidar(self):
        return self._download("lidar")

    def downloaded(self):
        """Names of the rasters a host consumer has pulled back so far."""
        return sorted(self._host)

    def get_data_shape(self):
        side = self.neighborhood * 2 + 1
        return [side, side, int(self.casi_dev.shape[2]) + (1 if self.lidar_dev is not None else 0)]

    def get_casi_band_count(self):
        return int(self.casi_dev.shape[2])

    def get_scene_shape(self):
        ref = self.lidar_dev if self.lidar_dev is not None else self.casi_dev
        return [int(ref.shape[0]) - 2 * self.neighborhood, int(ref.shape[1]) - 2 * self.neighborhood]


def device_shadow_ratio(data_set, shadow_map):
    """calculate_shadow_ratio for a device-resident scene: mean over the lit pixels / mean over the shadowed ones per
    band, formed in fp64 from the masked-sums launch and rounded to float32.  A pixel is in shadow where the map is
    non-zero, as in calculate_shadow_ratio (for a 0 / 1 map: map == 1).  Where one side of the map is empty the ratio is
    NaN (or inf); calculate_shadow_ratio reports numpy.ma's fill value (1e20) there instead -- neither is usable."""
    sums, counts = data_set.masked_band_sums(shadow_map)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        ratio = (sums[1] / counts[1]) / (sums[0] / counts[0])
    return ratio.astype(numpy.float32)
