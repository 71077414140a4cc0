"""TensorBoard event files without TensorFlow (reference classify/monitored_session_runner.py:16-28,
utilities/read_summary_file.py): the encoder and decoder of the few messages a classification run writes, TFRecord
framed through tfrecord_io.

Field numbers from TensorFlow's public event.proto, summary.proto, histogram.proto, tensor.proto, tensor_shape.proto:
    Event{wall_time=1 double, step=2 int64, file_version=3 string, summary=5}
    Summary{repeated value=1}; Summary.Value{tag=1, simple_value=2 float, histo=5, tensor=8, metadata=9}
    HistogramProto{min=1, max=2, num=3, sum=4, sum_squares=5 doubles, bucket_limit=6, bucket=7 packed doubles}
    TensorProto{dtype=1 (DT_STRING = 7), tensor_shape=2, string_val=8}; TensorShapeProto{repeated dim=2{size=1}}
    SummaryMetadata{plugin_data=1{plugin_name=1}}
Unpinned against TensorFlow itself (no TF-written file here), like the checkpoints; tests/test_tb_events.py parses the
writer's bytes with google.protobuf classes built from that schema.  The decoder skips unknown fields."""
import os
import socket
import struct
import sys
import time

import numpy

from hypelcnn_amd.common import tfrecord_io
from hypelcnn_amd.common.tf_checkpoint import _pb_bytes, _pb_fields, _pb_varint, put_varint

DT_STRING = 7
FILE_VERSION = "brain.Event:2"
DBL_MAX = sys.float_info.max


def default_bucket_limits():
    """tensorflow/core/lib/histogram/histogram.cc InitDefaultBucketsInner, in float64: 1e-12 * 1.1^k below 1e20, then
    DBL_MAX; the negatives mirrored, 0.0 in the middle (775 + 1 + 775 limits)."""
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(DBL_MAX)
    return numpy.asarray([-x for x in reversed(pos)] + [0.0] + pos, numpy.float64)


def _pb_double(field, v):
    return put_varint((field << 3) | 1) + struct.pack("<d", float(v))


def _pb_float(field, v):
    return put_varint((field << 3) | 5) + struct.pack("<f", float(v))


def _as_double(v):
    return struct.unpack("<d", struct.pack("<Q", v))[0]


def _as_int64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


# ------------------------------------------------------------------------------------------------ summary values
def scalar_value(tag, value):
    return _pb_bytes(1, tag.encode()) + _pb_float(2, value)


def _plugin_metadata(plugin_name):
    return _pb_bytes(9, _pb_bytes(1, _pb_bytes(1, plugin_name.encode())))


def text_value(tag, strings, shape=()):
    """A DT_STRING tensor summary of the "text" plugin: `strings` row-major, `shape` () for one string."""
    strings = [strings] if isinstance(strings, (str, bytes)) else list(strings)
    tensor = _pb_varint(1, DT_STRING)
    tensor += _pb_bytes(2, b"".join(_pb_bytes(2, _pb_varint(1, int(d))) for d in shape))
    tensor += b"".join(_pb_bytes(8, s if isinstance(s, bytes) else str(s).encode()) for s in strings)
    return _pb_bytes(1, tag.encode()) + _pb_bytes(8, tensor) + _plugin_metadata("text")


def matrix_text_value(tag, matrix):
    """An integer matrix as a [rows, cols] DT_STRING tensor of decimal strings (tf.as_string of the confusion matrix)."""
    m = numpy.asarray(matrix)
    return text_value(tag, [str(int(v)) for v in m.reshape(-1)], m.shape)


def collapse_buckets(limits, counts):
    """histogram.cc EncodeToProto(preserve_zero_buckets=false): a run of empty buckets becomes ONE entry with the limit
    of its last bucket and count 0, every non-empty bucket keeps its own (limit, count)."""
    out_l, out_c = [], []
    i, n = 0, len(counts)
    while i < n:
        end, count = limits[i], counts[i]
        i += 1
        if count <= 0:
            while i < n and counts[i] <= 0:
                end, count = limits[i], counts[i]
                i += 1
        out_l.append(float(end))
        out_c.append(float(count))
    return out_l, out_c


def histogram_value(tag, vmin, vmax, num, vsum, sum_squares, limits, counts):
    """limits / counts: the full bucket table; written collapsed (collapse_buckets)."""
    lim, cnt = collapse_buckets(limits, counts)
    histo = _pb_double(1, vmin) + _pb_double(2, vmax) + _pb_double(3, num) + _pb_double(4, vsum) + \
        _pb_double(5, sum_squares)
    histo += _pb_bytes(6, struct.pack(f"<{len(lim)}d", *lim)) + _pb_bytes(7, struct.pack(f"<{len(cnt)}d", *cnt))
    return _pb_bytes(1, tag.encode()) + _pb_bytes(5, histo)


def encode_event(wall_time, step, values=None, file_version=None):
    """values: encoded Summary.Value messages (scalar_value, text_value, histogram_value)."""
    out = _pb_double(1, wall_time) + _pb_varint(2, int(step))
    if file_version is not None:
        out += _pb_bytes(3, file_version.encode())
    if values is not None:
        out += _pb_bytes(5, b"".join(_pb_bytes(1, v) for v in values))
    return out


# ------------------------------------------------------------------------------------------------ decoding
def _doubles(wt, v):
    return list(struct.unpack(f"<{len(v) // 8}d", v)) if wt == 2 else [_as_double(v)]


def _decode_histogram(buf):
    h = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for field, wt, v in _pb_fields(buf):
        if field in names and wt == 1:
            h[names[field]] = _as_double(v)
        elif field == 6:
            h["bucket_limit"] += _doubles(wt, v)
        elif field == 7:
            h["bucket"] += _doubles(wt, v)
    return h


def _decode_tensor(buf):
    t = {"dtype": 0, "shape": [], "string_val": []}
    for field, wt, v in _pb_fields(buf):
        if field == 1 and wt == 0:
            t["dtype"] = v
        elif field == 2 and wt == 2:
            for f2, w2, dim in _pb_fields(v):
                if f2 == 2 and w2 == 2:
                    t["shape"].append(next((_as_int64(x) for f3, w3, x in _pb_fields(dim) if f3 == 1 and w3 == 0), 0))
        elif field == 8 and wt == 2:
            t["string_val"].append(v)
    return t


def _decode_value(buf):
    val = {"tag": ""}
    for field, wt, v in _pb_fields(buf):
        if field == 1 and wt == 2:
            val["tag"] = v.decode()
        elif field == 2 and wt == 5:
            val["simple_value"] = struct.unpack("<f", struct.pack("<I", v))[0]
        elif field == 5 and wt == 2:
            val["histo"] = _decode_histogram(v)
        elif field == 8 and wt == 2:
            val["tensor"] = _decode_tensor(v)
        elif field == 9 and wt == 2:
            for f2, w2, plugin in _pb_fields(v):
                if f2 == 1 and w2 == 2:
                    val["plugin_name"] = next((x.decode() for f3, w3, x in _pb_fields(plugin) if f3 == 1 and w3 == 2), "")
    return val


def decode_event(buf):
    """-> {"wall_time", "step", "file_version" (or None), "values": [{"tag", "simple_value" | "histo" | "tensor",
    "plugin_name"}]}"""
    ev = {"wall_time": 0.0, "step": 0, "file_version": None, "values": []}
    for field, wt, v in _pb_fields(buf):
        if field == 1 and wt == 1:
            ev["wall_time"] = _as_double(v)
        elif field == 2 and wt == 0:
            ev["step"] = _as_int64(v)
        elif field == 3 and wt == 2:
            ev["file_version"] = v.decode()
        elif field == 5 and wt == 2:
            ev["values"] += [_decode_value(x) for f2, w2, x in _pb_fields(v) if f2 == 1 and w2 == 2]
    return ev


def read_events(path, verify=True):
    """Yields the decoded events of one file; a truncated or corrupt record raises ValueError (TensorFlow's
    DataLossError) after the intact records before it were yielded."""
    records = tfrecord_io.read_records(path, verify=verify)
    while True:
        try:
            payload = next(records)
        except StopIteration:
            return
        except struct.error as e:  # a record cut inside its length / CRC words
            raise ValueError(f"{path}: truncated record ({e})") from e
        yield decode_event(payload)


# ------------------------------------------------------------------------------------------------ writer
class EventFileWriter:
    """events.out.tfevents.<unix seconds>.<hostname> in `log_dir`; the first record is the file_version event; every
    event is appended and flushed on its own."""

    def __init__(self, log_dir, now=None):
        os.makedirs(log_dir, exist_ok=True)
        now = time.time() if now is None else now
        self.path = os.path.join(log_dir, f"events.out.tfevents.{int(now):010d}.{socket.gethostname()}")
        self._append(encode_event(now, 0, file_version=FILE_VERSION))

    def _append(self, payload):
        with tfrecord_io._open(self.path, "ab", False) as f:
            tfrecord_io.write_record(f, payload)
            f.flush()

    def add_event(self, step, values, wall_time=None):
        self._append(encode_event(time.time() if wall_time is None else wall_time, step, values))
