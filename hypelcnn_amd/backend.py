"""ctypes binding of libhypel_hip.so (include/hypel.h) -- the only compute backend of the product.

There is deliberately NO CPU fallback here: if the HIP library is missing or there is no GPU,
`HipBackend()` raises.  (tests/ inject a numpy emulation of this same interface to exercise the
host-side planner without a GPU; that emulation lives under tests/, not in the package.)

A backend exposes one method per C-ABI entry point.  Pointer arguments are `Ref`s
(flat torch tensor + element offset); `bind(name, args)` resolves them once and returns a
zero-argument callable, so a planned step is replayed as a flat list of pre-bound C calls.
"""
import ctypes
import os
import time
import subprocess

import numpy as np
import torch

from . import abi
from .abi import HypelError  # noqa: F401 (raised here, imported from here by the rest of the package)

_HERE = os.path.dirname(os.path.abspath(__file__))
# HYPEL_LIB_PATH: an alternative build of the same ABI (A/B experiments on one GPU box)
LIB_PATH = os.environ.get("HYPEL_LIB_PATH") or os.path.join(_HERE, "csrc", "libhypel_hip.so")

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_SIGMOID, ACT_TANH = (abi.const("HYPEL_ACT_" + k)
                                                         for k in ("NONE", "LRELU", "RELU", "SIGMOID", "TANH"))
GEMM_BM = abi.const("HYPEL_GEMM_BM")
ABI_VERSION = abi.const("HYPEL_ABI_VERSION")  # a library built from other headers is refused at load time

SEG_DTYPE = abi.struct("hypel_seg_t")
GROUP_DTYPE = abi.struct("hypel_group_t")
TILE_DTYPE = abi.struct("hypel_tile_t")
MTILE_DTYPE = abi.struct("hypel_mtile_t")
REDUCE_ENTRY_DTYPE = abi.struct("hypel_reduce_entry_t")
COPY_BLOCK_DTYPE = abi.struct("hypel_copy_block_t")
LOSS_TERM_DTYPE = abi.struct("hypel_loss_term_t")
LOSS_NONE = abi.const("HYPEL_LOSS_NONE")
TILE_PLAIN = abi.const("HYPEL_TILE_PLAIN")  # K-slice partial (no bias / accumulate / shortcut gather)
# output dtypes of hypel_denorm_scatter, input dtypes of hypel_hsi_to_srgb
OUT_DTYPES = {np.dtype(t): abi.const("HYPEL_DTYPE_" + k)
              for t, k in ((np.float32, "F32"), (np.uint16, "U16"), (np.int16, "I16"), (np.uint8, "U8"))}
RGB_U8, RGB_F32 = abi.const("HYPEL_RGB_U8"), abi.const("HYPEL_RGB_F32")  # output modes of hypel_hsi_to_srgb
SVM_PAIR_DTYPE = abi.struct("hypel_svm_pair_t")
SVM_JOB_DTYPE = abi.struct("hypel_svm_job_t")  # a pair + the element offset of its plane of K + its C (hypel_svm_smo_grid)
SVM_RBF, SVM_POLY = abi.const("HYPEL_SVM_RBF"), abi.const("HYPEL_SVM_POLY")
SVM_CONVERGED, SVM_NOT_CONVERGED = abi.const("HYPEL_SVM_CONVERGED"), abi.const("HYPEL_SVM_NOT_CONVERGED")
SVM_MAX_ITER_LIMIT = abi.const("HYPEL_SVM_MAX_ITER_LIMIT")
SCENE_RANK_WS_WORDS = abi.const("HYPEL_SCENE_RANK_WS_WORDS")  # uint32 of workspace per band
# uint32 of workspace per band and ranks per call of hypel_column_rank_select_f32
COLUMN_RANK_WS_WORDS, COLUMN_RANK_MAX_RANKS, COLUMN_RANK_MAX_BANDS = (
    abi.const("HYPEL_COLUMN_RANK_" + k) for k in ("WS_WORDS", "MAX_RANKS", "MAX_BANDS"))
COMPACT_TILE = abi.const("HYPEL_COMPACT_TILE")  # pixels per int32 of hypel_mask_compact_points_i32's workspace
# classes of hypel_components_votes_i32 (its exclude mask is 64 bits), status words of hypel_components_label_u8
COMPONENTS_MAX_CLASSES = abi.const("HYPEL_COMPONENTS_MAX_CLASSES")
COMPONENTS_OK, COMPONENTS_STEP_CAP = abi.const("HYPEL_COMPONENTS_OK"), abi.const("HYPEL_COMPONENTS_STEP_CAP")
# hypel_match_ccorr_f32: side of an output tile, image rows and template columns of one staged chunk, output columns of a
# block, and the most column-chunk splits a call takes
MATCH_TILE, MATCH_ROW_CHUNK, MATCH_COL_CHUNK, MATCH_BLOCK_COLS, MATCH_MAX_SPLITS = (
    abi.const("HYPEL_MATCH_" + k) for k in ("TILE", "ROW_CHUNK", "COL_CHUNK", "BLOCK_COLS", "MAX_SPLITS"))
SUMMARY_SLICE = abi.const("HYPEL_SUMMARY_SLICE")  # elements per slice of hypel_tensor_summary_f32
SUMMARY_MAX_LIMITS = abi.const("HYPEL_SUMMARY_MAX_LIMITS")
ACT_MAX_BINS = abi.const("HYPEL_ACT_MAX_BINS")  # bins of hypel_view_histogram_f32 (its LDS table and histogram)
# rows sorted per column for the bin edges, edges per column, classes of the LDS histogram, depth cap of the level loop
FOREST_EDGE_ROWS, FOREST_MAX_EDGES, FOREST_MAX_CLASSES, FOREST_MAX_DEPTH = (
    abi.const("HYPEL_FOREST_" + k) for k in ("EDGE_ROWS", "MAX_EDGES", "MAX_CLASSES", "MAX_DEPTH"))
FOREST_NODE_DTYPE = abi.struct("hypel_forest_node_t")  # a leaf has left = -1 - (its row of the leaf table)
# hypel_pca_*: most bands, pixels per float32 accumulator, side of a scatter tile, most blocks of a fit pass
PCA_MAX_BANDS, PCA_CHUNK, PCA_TILE, PCA_MAX_BLOCKS = (abi.const("HYPEL_PCA_" + k)
                                                      for k in ("MAX_BANDS", "CHUNK", "TILE", "MAX_BLOCKS"))
# hypel_morph_*: largest radius of a structuring element, most blocks of a launch, the raster kernels' tile, shapes, ops
MORPH_MAX_RADIUS, MORPH_MAX_BLOCKS, MORPH_TILE_W, MORPH_TILE_H, MORPH_DISK, MORPH_SQUARE, MORPH_ERODE, MORPH_DILATE = (
    abi.const("HYPEL_MORPH_" + k) for k in ("MAX_RADIUS", "MAX_BLOCKS", "TILE_W", "TILE_H", "DISK", "SQUARE", "ERODE", "DILATE"))
TIFF_SEG_DTYPE = abi.struct("hypel_tiff_seg_t")  # byte offsets and lengths
TIFF_LZW, TIFF_PACKBITS = abi.const("HYPEL_TIFF_LZW"), abi.const("HYPEL_TIFF_PACKBITS")  # codecs of hypel_tiff_unpack


class Ref:
    """A device (or, for the test emulation, host) address: flat tensor + element offset."""
    __slots__ = ("t", "off")

    def __init__(self, t, off=0):
        self.t = t
        self.off = int(off)

    def ptr(self):
        return self.t.data_ptr() + self.off * self.t.element_size()

    def __add__(self, elems):
        return Ref(self.t, self.off + int(elems))


def build_library(verbose=False):
    """Compile libhypel_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4", "libhypel_hip.so"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_P = ctypes.c_void_p

# launch entry points (last parameter `hypel_stream_t stream`; the hypel_graph_* calls control a capture and are no
# launches): short name -> argument ctypes without the stream
SIGNATURES = {name[len("hypel_"):]: [t for _, t in params[:-1]] for name, (_, params) in abi.FUNCTIONS.items()
              if params and params[-1][0] == "stream" and not name.startswith("hypel_graph_")}


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise HypelError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (restype, params) in abi.FUNCTIONS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            continue  # optional entry points (checked by tests/test_abi.py against the header)
        fn.argtypes = [t for _, t in params]
        fn.restype = restype
    return lib


# host-side pseudo-launches of a plan (bind_collective) and their parameter names
COLLECTIVES = {"_allreduce": ("ref", "count"), "_allgather": ("src", "count", "dst")}


def arg_index(name, param):
    """Position of the header's parameter `param` in the argument tuple of a `name` launch."""
    names = COLLECTIVES.get(name) or [p for p, _ in abi.FUNCTIONS["hypel_" + name][1]]
    if param not in names:
        raise HypelError(f"hypel_{name} has no parameter {param!r}: its parameters are ({', '.join(names)})")
    return names.index(param)


def bind_collective(name, args):
    """Host-side pseudo-launches of a plan (synchronised batch norm): `_allreduce (ref, count)` sums `count` floats in
    place over the data-parallel ranks, `_allgather (src, count, dst)` writes every rank's `count` floats to
    dst[rank * count ...].  torch.distributed orders them with the current stream (RCCL on the GPU box, gloo in the CPU
    tests); they cannot be captured, so a compiled tower cuts its HIP graphs around them (`host` attribute)."""
    import torch.distributed as dist
    if name == "_allreduce":
        ref, count = args

        def call():
            note_collective()
            dist.all_reduce(ref.t[ref.off:ref.off + count], op=dist.ReduceOp.SUM)
    else:
        src, count, dst = args

        def call():
            # into ONE long-lived tensor: the list form of all_gather stages through a temporary whose release (by the
            # process group's watchdog thread, whenever it reaps the finished work) makes the caching allocator record
            # and poll an event -- which invalidates a HIP-graph capture that happens to be under way on the compute
            # stream ("operation not permitted on an event last recorded in a capturing stream", 1 run in 8)
            world = dist.get_world_size()
            note_collective()
            dist.all_gather_into_tensor(dst.t[dst.off:dst.off + world * count], src.t[src.off:src.off + count])

    call.host = True
    return call


_collective_epoch = [0]  # bumped by every collective the package issues (note_collective)


def _pg_sequence_number():
    """Collective sequence number of the default process group (None when the build does not expose it): moves with
    every collective issued on it, whoever issued it."""
    try:
        import torch.distributed as dist
        return int(dist.distributed_c10d._get_default_group()._get_sequence_number_for_group())
    except Exception:  # noqa: BLE001 -- private API: absent / renamed means "unknown", the package epoch still counts
        return None


def note_collective():
    """Called right before any torch.distributed collective of the package: a HIP-graph capture must not start while
    the RCCL watchdog still polls that collective (HipBackend.settle_before_capture waits it out -- once per burst of
    captures, not once per capture, as long as no collective was issued in between)."""
    _collective_epoch[0] += 1


class HipBackend:
    """Launches hand-written gfx950 kernels through the C-ABI on a torch CUDA(HIP) stream."""
    name = "hip"
    _settled_epoch = -1  # value of the collective epoch at the last settle_before_capture() pause
    _streams = {}  # device index -> (main stream, side stream), shared by every backend object of the process

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise HypelError("no HIP device visible: the hypelcnn_amd compute path needs an MI355X "
                             "(there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.lib = load_library()
        if self.lib.hypel_version() != ABI_VERSION:
            raise HypelError(f"libhypel_hip.so ABI version {self.lib.hypel_version()} != {ABI_VERSION} (stale build or HYPEL_LIB_PATH)")
        # All hypel launches (and the torch plumbing ops around them) run on ONE dedicated non-default
        # stream: HIP cannot capture the legacy null stream into a graph, and a private stream keeps the
        # step ordered without device-wide syncs.  The stream is per DEVICE, not per backend object: torch's
        # "current stream" is process-global state, so a second HipBackend with streams of its own would silently
        # move the first one's copies (set_input, .cpu()) onto a stream its kernels are not ordered with.
        key = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if key not in HipBackend._streams:
            HipBackend._streams[key] = torch.cuda.Stream(self.device)
        self.stream = HipBackend._streams[key]
        torch.cuda.set_stream(self.stream)

    # -- memory (PyTorch is the allocator: plumbing only) --
    def empty(self, n, dtype=torch.float32):
        return torch.empty(int(n), dtype=dtype, device=self.device)

    def zeros(self, n, dtype=torch.float32):
        t = torch.empty(int(n), dtype=dtype, device=self.device)
        nbytes = t.numel() * t.element_size()
        if nbytes == 0:
            return t
        if nbytes % 4:  # (byte tables of odd length: not on any step path)
            return t.zero_()
        self.call("fill_f32", Ref(t.view(torch.uint8).view(torch.float32)), nbytes // 4, 0.0)  # hypel_fill, not a torch kernel
        return t

    def upload(self, array):
        """numpy array (any dtype, incl. structured tables) -> flat device tensor."""
        a = np.ascontiguousarray(array)
        if a.dtype.fields is not None:
            t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy())
        else:
            t = torch.from_numpy(a.reshape(-1).copy())
        return t.to(self.device)

    def stream_handle(self):
        return self.stream.cuda_stream

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    def gan_generator_blocks(self, n):
        return int(self.lib.hypel_gan_generator_blocks(int(n)))

    def dense_stack_blocks(self, n):
        return int(self.lib.hypel_dense_stack_blocks(int(n)))

    def gan_generator_blocks_apps(self, n, n_apps):
        return int(self.lib.hypel_gan_generator_blocks_apps(int(n), int(n_apps)))

    def dense_stack_blocks_apps(self, n, n_apps):
        return int(self.lib.hypel_dense_stack_blocks_apps(int(n), int(n_apps)))

    def dense_stack_supported(self, widths):
        w = list(widths) + [0] * (5 - len(widths))
        return len(widths) <= 5 and bool(self.lib.hypel_dense_stack_supported(len(widths) - 1, *[int(v) for v in w]))

    def gan_generator_tap_supported(self, bands):
        return bool(self.lib.hypel_gan_generator_tap_supported(int(bands)))

    def gan_generator_keep_floats(self, n, bands, only_encoder):
        return int(self.lib.hypel_gan_generator_keep_floats(int(n), int(bands), int(only_encoder)))

    # -- launches --
    def bind(self, name, args, stream=None):
        if name in COLLECTIVES:
            return bind_collective(name, args)
        fn = getattr(self.lib, "hypel_" + name)
        st = self.stream_handle() if stream is None or stream == 0 else stream
        cargs = []
        for a in args:
            if isinstance(a, Ref):
                cargs.append(a.ptr())
            elif a is None:
                cargs.append(None)
            else:
                cargs.append(a)
        cargs.append(st)
        cargs = tuple(cargs)
        lib = self.lib

        def call():
            rc = fn(*cargs)
            if rc != 0:
                raise HypelError(f"hypel_{name} failed ({rc}): {lib.hypel_last_error().decode()}")

        return call

    def call(self, name, *args):
        self.bind(name, args)()

    # -- HIP graph capture --
    def settle_before_capture(self):
        """A HIP-graph capture on the compute stream must not overlap the RCCL process group's watchdog thread while
        that thread still polls / reaps finished collectives: HIP then fails the capture AND the watchdog's event query
        ("operation not permitted on an event last recorded in a capturing stream", which terminates the process).
        torch.cuda.graph() coordinates with the watchdog internally; a capture started through the C-ABI cannot, so it
        waits until the device is idle and the watchdog (100 ms period) has nothing left to look at.  Reproduced and
        cured in tools/exp/capture_vs_watchdog.py: 8 of 9 runs of 60 capture bursts die without the pause, 0 of 6 with
        it.  No-op without an initialised NCCL process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_backend() != "nccl":
            return
        # "anything issued since the last pause?" = the package's own epoch (note_collective) AND the process group's
        # collective sequence number, which also moves for dist.* calls made outside the package (bench.py, user code);
        # HYPEL_CAPTURE_SETTLE_ALWAYS=1 pauses before every capture regardless
        epoch = (_collective_epoch[0], _pg_sequence_number())
        if os.environ.get("HYPEL_CAPTURE_SETTLE_ALWAYS") != "1" and HipBackend._settled_epoch == epoch:
            return  # no collective since the last pause: the watchdog has nothing new to poll (a burst of captures --
            #         every batch size of a run, TrainStep.precapture -- pays the pause once)
        torch.cuda.synchronize(self.device)
        time.sleep(float(os.environ.get("HYPEL_CAPTURE_SETTLE_S", "0.5")))
        HipBackend._settled_epoch = (_collective_epoch[0], _pg_sequence_number())

    def capture(self, launches, settled=False):
        """Capture a list of bound launches into a hipGraphExec; returns a replay callable.
        settled: the caller already called settle_before_capture() and issued no collective since."""
        if not settled:
            self.settle_before_capture()
        st = self.stream_handle()
        lib = self.lib
        if lib.hypel_graph_begin_capture(st) != 0:
            raise HypelError(lib.hypel_last_error().decode())
        try:
            for f in launches:
                f()
        finally:
            exec_ = _P()
            rc = lib.hypel_graph_end_capture(st, ctypes.byref(exec_))
        if rc != 0:
            raise HypelError(lib.hypel_last_error().decode())
        handle = exec_.value

        def replay():
            if lib.hypel_graph_launch(handle, st) != 0:
                raise HypelError(lib.hypel_last_error().decode())

        replay.handle = handle
        return replay

    def destroy_graph(self, replay):
        """Give a captured graph back to the runtime (hipGraphExecDestroy).  The caller has synchronised: no replay of
        it is in flight, and it is not replayed again."""
        handle, replay.handle = getattr(replay, "handle", None), None
        if handle:
            self.lib.hypel_graph_destroy(handle)
