#!/usr/bin/env python3
"""Times the TIFF device path (common/tiff_io.read_raster, csrc/tiff.hip) step by step on synthetic rasters of the
contest scenes' sizes -- a 1202 x 4768 x 50 uint16 scene and a 2404 x 8344 float32 LiDAR raster -- written in the
layouts real files come in, beside the byte floors of the two launches (unpack: stream read + decoded bytes written;
assemble: decoded bytes read + raster written) and the host imread for scale.  Needs a HIP device.

    python tools/tiff_bench.py [--reps 3] [--skip-host] [--small] [--dir DIR]
prints one JSON line per file.  The files are written by tests/tiff_cases.write_tiff; the rasters are periodic with
the tile size, so that its plain-Python LZW encoder runs once per distinct tile (lzw_cache); the host imread is not
timed for LZW files (plain Python: minutes)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common import tiff_io as T  # noqa: E402
from tests.tiff_cases import write_tiff  # noqa: E402  (the one TIFF writer of the repository: the tests' own)

HBM_GBS = 6290.0  # measured float4 copy rate of the MI355X, the ceiling the floors are quoted against
TILE = 256


def timed(be, fn, reps):
    fn()
    be.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def step(ms, nbytes):
    return {"ms": round(ms, 3), "floor_ms": round(nbytes / HBM_GBS / 1e6, 3), "GBps": round(nbytes / ms / 1e6, 1)}


def case(be, name, path, pixels, reps, skip_host):
    lay, parse_ms = wall(lambda: T.read_layout(path))
    rec = {"case": name, "shape": list(lay.shape), "dtype": str(lay.dtype), "file_MB": round(lay.file_size / 1e6, 1),
           "segments": lay.n_segments, "parse_ms": round(parse_ms, 2), "in_place": lay.in_place}
    buf = np.fromfile(path, np.uint8)
    raster_bytes = lay.height * lay.width * lay.spp * lay.item
    if lay.in_place:
        def up():
            t = be.upload(buf[lay.offsets[0]:lay.offsets[0] + raster_bytes])
            be.synchronize()
            return t
        dev, ms = wall(up)
        rec["upload"] = {"ms": round(ms, 1), "GBps": round(raster_bytes / ms / 1e6, 1)}
        got = T.DeviceRaster(dev, 0, lay.dtype, lay.shape)
    else:
        table, dst_bytes = T.segment_table(lay)
        T.check_segment_table(table, len(buf), dst_bytes)
        host_src = buf
        if lay.compression == T.COMPRESSION_DEFLATE:
            def inflate():
                host = np.zeros(dst_bytes, np.uint8)
                for r, seg in zip(table, T._decode_all(buf, lay)):
                    host[r["dst_off"]:r["dst_off"] + r["dst_len"]] = np.frombuffer(seg, np.uint8)
                return host
            host_src, ms = wall(inflate)
            rec["host_inflate_ms"] = round(ms, 1)

        def up():
            t = be.upload(host_src)
            be.synchronize()
            return t
        src, ms = wall(up)
        rec["upload"] = {"ms": round(ms, 1), "GBps": round(len(host_src) / ms / 1e6, 1)}
        table_dev = be.upload(table)
        if lay.compression in (T.COMPRESSION_LZW, T.COMPRESSION_PACKBITS):
            decoded = be.empty(dst_bytes, torch.uint8)
            status = be.zeros(lay.n_segments, torch.int32)
            ms = timed(be, lambda: be.call("tiff_unpack", Ref(src), len(buf), Ref(table_dev), lay.n_segments,
                                           lay.compression, Ref(decoded), dst_bytes, Ref(status)), reps)
            T.raise_for_status(status.cpu().numpy())
            rec["unpack"] = step(ms, int(sum(lay.counts)) + int(table["dst_len"].sum()))
            src = decoded
        out = be.empty(raster_bytes, torch.uint8)
        ms = timed(be, lambda: be.call(
            "tiff_assemble", Ref(src), int(src.numel()), Ref(table_dev), lay.n_segments,
            int(lay.compression != T.COMPRESSION_NONE), lay.height, lay.width, lay.spp, lay.item, lay.seg_rows,
            lay.seg_cols, lay.segs_across, lay.planes, lay.predictor, int(lay.byteorder == "MM"), Ref(out)), reps)
        rec["assemble"] = step(ms, int(table["dst_len"].sum()) + raster_bytes)
        got = T.DeviceRaster(out, 0, lay.dtype, lay.shape)
    rec["correct"] = bool(np.array_equal(got.download(), pixels))
    del got
    _, ms = wall(lambda: T.read_raster(path, be))
    rec["read_raster_ms"] = round(ms, 1)
    if not skip_host and lay.compression != T.COMPRESSION_LZW:
        host, ms = wall(lambda: T.imread(path))
        rec["host_imread_ms"] = round(ms, 1)
        rec["host_correct"] = bool(np.array_equal(host, pixels))
    print(json.dumps(rec), flush=True)


def periodic(shape, dtype, rng):
    """a raster whose every TILE x TILE tile holds the same samples: smooth along x with a few levels of noise"""
    h, w = shape[:2]
    bands = shape[2] if len(shape) == 3 else 1
    xx = np.arange(TILE)
    base = 2000 + 900 * np.sin(xx / 40.0)[None, :, None] + 37 * np.arange(bands)[None, None, :]
    tile = base + rng.integers(-8, 9, (TILE, TILE, bands))
    tile = tile.astype(dtype) if np.dtype(dtype).kind != "f" else (tile * 0.0137).astype(dtype)
    full = np.tile(tile, (-(-h // TILE), -(-w // TILE), 1))[:h, :w]
    return np.ascontiguousarray(full if len(shape) == 3 else full[:, :, 0])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--small", action="store_true", help="a tenth of the rows: a quick look")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args(argv)
    be = HipBackend()
    rng = np.random.default_rng(0)
    cut = 10 if a.small else 1
    rasters = [("scene", periodic((1202 // cut, 4768, 50), np.uint16, rng), 2),
               ("lidar", periodic((2404 // cut, 8344), np.float32, rng), 3)]
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for label, px, deflate_predictor in rasters:
            layouts = [("one strip", {}), ("one row per strip", {"rows_per_strip": 1}),
                       ("256x256 tiles", {"tile": (TILE, TILE)}),
                       ("tiles + LZW + predictor 2", {"tile": (TILE, TILE), "compression": 5, "predictor": 2}),
                       (f"16-row strips + Deflate + predictor {deflate_predictor}",
                        {"rows_per_strip": 16, "compression": 8, "predictor": deflate_predictor}),
                       ("one row per strip, big-endian", {"rows_per_strip": 1, "order": ">"})]
            if px.ndim == 3:
                layouts.insert(5, ("band-sequential planes, 16-row strips", {"rows_per_strip": 16, "planar": 2}))
            for name, kw in layouts:
                path = os.path.join(d, "bench.tif")
                write_tiff(path, px, zlib_level=1, workers=T.POOL_WORKERS, lzw_cache={}, **kw)
                case(be, f"{label} {'x'.join(map(str, px.shape))} {px.dtype}: {name}", path, px, a.reps, a.skip_host)
                os.remove(path)


if __name__ == "__main__":
    main()
