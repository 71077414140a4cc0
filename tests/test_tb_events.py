"""CPU: TensorBoard event files of common/tb_events.py -- the default bucket table, the encoder against an independent
decoder (google.protobuf classes built here from TensorFlow's public schema), known-answer bytes, TFRecord framing and
the truncated-file branch of utilities/read_summary_file."""
import os
import struct
import sys

import numpy as np
import pytest

from hypelcnn_amd.common import tb_events, tfrecord_io

DBL_MAX = sys.float_info.max
FLT_MAX = float(np.finfo(np.float32).max)


# ----------------------------------------------------------------------------- bucket table
def test_default_bucket_table():
    lim = tb_events.default_bucket_limits()
    assert lim.dtype == np.float64 and lim.size == 1551 and (np.diff(lim) > 0).all()
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[-1] == DBL_MAX and lim[0] == -DBL_MAX
    assert np.array_equal(lim[:775], -lim[:775:-1])

    def bucket(v):
        return int(np.searchsorted(lim, np.float64(np.float32(v)), side="right"))

    assert bucket(0.0) == 776 and bucket(-0.0) == 776 and bucket(1e-45) == 776
    assert bucket(FLT_MAX) == 1550 and bucket(-FLT_MAX) == 1


def test_zero_bucket_runs_collapse():
    limits = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert tb_events.collapse_buckets(limits, [0, 0, 3, 0, 0, 0, 2]) == ([2.0, 3.0, 6.0, 7.0], [0.0, 3.0, 0.0, 2.0])
    assert tb_events.collapse_buckets(limits, [1, 2, 0, 4, 0, 0, 0]) == ([1.0, 2.0, 3.0, 4.0, 7.0],
                                                                         [1.0, 2.0, 0.0, 4.0, 0.0])
    assert tb_events.collapse_buckets(limits, [0] * 7) == ([7.0], [0.0])


# ----------------------------------------------------------------------------- independent decoder
@pytest.fixture(scope="module")
def pb():
    """Event and its parts as google.protobuf message classes, from a FileDescriptorProto that states the schema"""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="tb_events_test.proto", package="tbt", syntax="proto3")

    def message(parent, name, fields):
        m = parent.message_type.add() if parent is fd else parent.nested_type.add()
        m.name = name
        for fname, number, ftype, label, type_name in fields:
            f = m.field.add(name=fname, number=number, type=ftype, label=label)
            if type_name:
                f.type_name = type_name
        return m

    one, many = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    message(fd, "HistogramProto", [("min", 1, F.TYPE_DOUBLE, one, ""), ("max", 2, F.TYPE_DOUBLE, one, ""),
                                   ("num", 3, F.TYPE_DOUBLE, one, ""), ("sum", 4, F.TYPE_DOUBLE, one, ""),
                                   ("sum_squares", 5, F.TYPE_DOUBLE, one, ""),
                                   ("bucket_limit", 6, F.TYPE_DOUBLE, many, ""), ("bucket", 7, F.TYPE_DOUBLE, many, "")])
    shape = message(fd, "TensorShapeProto", [("dim", 2, F.TYPE_MESSAGE, many, ".tbt.TensorShapeProto.Dim")])
    message(shape, "Dim", [("size", 1, F.TYPE_INT64, one, "")])
    message(fd, "TensorProto", [("dtype", 1, F.TYPE_INT32, one, ""),
                                ("tensor_shape", 2, F.TYPE_MESSAGE, one, ".tbt.TensorShapeProto"),
                                ("string_val", 8, F.TYPE_BYTES, many, "")])
    meta = message(fd, "SummaryMetadata", [("plugin_data", 1, F.TYPE_MESSAGE, one, ".tbt.SummaryMetadata.PluginData")])
    message(meta, "PluginData", [("plugin_name", 1, F.TYPE_STRING, one, "")])
    summary = message(fd, "Summary", [("value", 1, F.TYPE_MESSAGE, many, ".tbt.Summary.Value")])
    message(summary, "Value", [("tag", 1, F.TYPE_STRING, one, ""), ("simple_value", 2, F.TYPE_FLOAT, one, ""),
                               ("histo", 5, F.TYPE_MESSAGE, one, ".tbt.HistogramProto"),
                               ("tensor", 8, F.TYPE_MESSAGE, one, ".tbt.TensorProto"),
                               ("metadata", 9, F.TYPE_MESSAGE, one, ".tbt.SummaryMetadata")])
    message(fd, "Event", [("wall_time", 1, F.TYPE_DOUBLE, one, ""), ("step", 2, F.TYPE_INT64, one, ""),
                          ("file_version", 3, F.TYPE_STRING, one, ""), ("summary", 5, F.TYPE_MESSAGE, one, ".tbt.Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("tbt.Event"))


def _sample_histogram():
    lim = tb_events.default_bucket_limits()
    counts = np.zeros(lim.size, np.int64)
    counts[[3, 700, 701, 776, 900, 1550]] = [5, 1, 2, 40, 7, 1]
    return lim, counts


def test_writer_round_trips_through_protobuf(pb, tmp_path):
    lim, counts = _sample_histogram()
    confusion = np.asarray([[5, 0, 1], [2, 70000, 0], [0, 3, 9]])
    w = tb_events.EventFileWriter(str(tmp_path), now=1700000000.25)
    assert os.path.basename(w.path).startswith("events.out.tfevents.1700000000.")
    w.add_event(7, [tb_events.scalar_value("training_cross_entropy", 0.1),
                    tb_events.scalar_value("validation_kappa", -0.25),
                    tb_events.matrix_text_value("validation_confusion", confusion),
                    tb_events.text_value("flags", "<pre>{\n \"a\": 1\n}</pre>"),
                    tb_events.histogram_value("nn_core/w", -1.5, 2.5, 56.0, 3.25, 9.125, lim, counts)], wall_time=12.5)
    w.add_event(2 ** 40 + 1, [], wall_time=13.0)
    records = list(tfrecord_io.read_records(w.path, verify=True))  # framing and both CRCs
    assert len(records) == 3
    first, ev, big = (pb.FromString(r) for r in records)
    assert first.file_version == "brain.Event:2" and first.wall_time == 1700000000.25 and first.step == 0
    assert not first.HasField("summary")
    assert big.step == 2 ** 40 + 1 and big.wall_time == 13.0 and len(big.summary.value) == 0
    assert ev.step == 7 and ev.wall_time == 12.5 and ev.file_version == ""
    v = ev.summary.value
    assert [x.tag for x in v] == ["training_cross_entropy", "validation_kappa", "validation_confusion", "flags",
                                  "nn_core/w"]
    assert v[0].simple_value == float(np.float32(0.1)) and v[1].simple_value == -0.25  # scalars are float32
    t = v[2].tensor
    assert t.dtype == 7 and [d.size for d in t.tensor_shape.dim] == [3, 3]
    assert [s.decode() for s in t.string_val] == [str(x) for x in confusion.reshape(-1)]
    assert v[2].metadata.plugin_data.plugin_name == "text" and v[3].metadata.plugin_data.plugin_name == "text"
    assert len(v[3].tensor.tensor_shape.dim) == 0 and list(v[3].tensor.string_val) == [b"<pre>{\n \"a\": 1\n}</pre>"]
    h = v[4].histo
    assert (h.min, h.max, h.num, h.sum, h.sum_squares) == (-1.5, 2.5, 56.0, 3.25, 9.125)
    # zero runs collapsed: [0..2] -> limit[2], 3, [4..699] -> limit[699], 700, 701, [702..775], 776, ...
    want = [(lim[2], 0), (lim[3], 5), (lim[699], 0), (lim[700], 1), (lim[701], 2), (lim[775], 0), (lim[776], 40),
            (lim[899], 0), (lim[900], 7), (lim[1549], 0), (lim[1550], 1)]
    assert list(zip(h.bucket_limit, h.bucket)) == [(float(a), float(b)) for a, b in want]
    # and the package's own decoder reads the same
    own = list(tb_events.read_events(w.path))
    assert own[0]["file_version"] == "brain.Event:2" and own[1]["step"] == 7 and own[2]["step"] == 2 ** 40 + 1
    ov = own[1]["values"]
    assert ov[0]["simple_value"] == v[0].simple_value and ov[2]["tensor"]["shape"] == [3, 3]
    assert ov[2]["plugin_name"] == "text" and ov[2]["tensor"]["string_val"] == list(t.string_val)
    assert ov[4]["histo"]["bucket_limit"] == list(h.bucket_limit) and ov[4]["histo"]["bucket"] == list(h.bucket)
    assert ov[4]["histo"]["sum_squares"] == 9.125


def test_protobuf_written_events_decode(pb):
    """the other direction: what google.protobuf serialises, the package's decoder reads (unknown fields skipped)"""
    ev = pb(wall_time=3.5, step=-4)
    val = ev.summary.value.add(tag="x", simple_value=1.25)
    val.histo.bucket_limit.extend([1.0, 2.0])
    val.histo.bucket.extend([3.0, 4.0])
    val.histo.num = 7.0
    data = ev.SerializeToString() + bytes([0x90, 0x06, 0x01])  # + an unknown varint field 98
    got = tb_events.decode_event(data)
    assert got["wall_time"] == 3.5 and got["step"] == -4 and got["values"][0]["simple_value"] == 1.25
    assert got["values"][0]["histo"]["bucket_limit"] == [1.0, 2.0] and got["values"][0]["histo"]["num"] == 7.0


# ----------------------------------------------------------------------------- known-answer bytes
def test_known_answer_bytes():
    d = lambda *xs: struct.pack(f"<{len(xs)}d", *xs)  # noqa: E731
    scalar = tb_events.encode_event(1.5, 3, [tb_events.scalar_value("a", 0.5)])
    assert scalar.hex() == "09000000000000f83f" "1003" "2a0a" "0a08" "0a0161" "150000003f"
    histo = tb_events.encode_event(2.0, 7, [tb_events.histogram_value("h", 0.5, 2.5, 3, 5.5, 12.75, [1.0, 2.0, 3.0],
                                                                        [1, 0, 2])])
    body = b"\x09" + d(0.5) + b"\x11" + d(2.5) + b"\x19" + d(3.0) + b"\x21" + d(5.5) + b"\x29" + d(12.75) + \
        b"\x32\x18" + d(1.0, 2.0, 3.0) + b"\x3a\x18" + d(1.0, 0.0, 2.0)
    assert len(body) == 0x61
    assert histo == b"\x09" + d(2.0) + b"\x10\x07" + b"\x2a\x68" + b"\x0a\x66" + b"\x0a\x01h" + b"\x2a\x61" + body
    version = tb_events.encode_event(0.0, 0, file_version="brain.Event:2")
    assert version == b"\x09" + d(0.0) + b"\x10\x00" + b"\x1a\x0dbrain.Event:2"


def test_tfrecord_framing_of_the_event_file(tmp_path):
    w = tb_events.EventFileWriter(str(tmp_path), now=5.0)
    w.add_event(1, [tb_events.scalar_value("a", 0.5)], wall_time=1.5)
    raw = open(w.path, "rb").read()
    first = tb_events.encode_event(5.0, 0, file_version="brain.Event:2")
    assert struct.unpack_from("<Q", raw, 0)[0] == len(first) and raw[12:12 + len(first)] == first
    assert len(raw) == 16 + len(first) + 16 + 23
    assert os.path.basename(w.path).split(".")[3] == "0000000005"
    assert [len(r) for r in tfrecord_io.read_records(w.path, verify=True)] == [len(first), 23]
    flipped = bytearray(raw)
    flipped[14] ^= 1
    open(w.path, "wb").write(flipped)
    with pytest.raises(ValueError):
        list(tfrecord_io.read_records(w.path, verify=True))


# ----------------------------------------------------------------------------- corruption
@pytest.mark.parametrize("cut", [1, 6, 30])
def test_truncated_last_record_is_reported_and_skipped(tmp_path, capsys, cut):
    from hypelcnn_amd.utilities import read_summary_file
    log_dir = tmp_path / "exp" / "run1"
    w = tb_events.EventFileWriter(str(log_dir), now=9.0)
    a, b = np.asarray([[3, 1], [0, 4]]), np.asarray([[2, 2], [1, 3]])
    w.add_event(10, [tb_events.matrix_text_value("validation_confusion", a)])
    w.add_event(20, [tb_events.matrix_text_value("validation_confusion", b)])
    raw = open(w.path, "rb").read()
    open(w.path, "wb").write(raw[:-cut])  # inside the payload CRC, the payload, and further up
    found = read_summary_file.read_confusions(str(log_dir), out_dir=str(tmp_path))
    out = capsys.readouterr().out
    assert "Error reading summary file" in out and w.path in out
    assert [(s, os.path.basename(p)) for s, p, _ in found] == [(10, "exp_run1_s10.csv")]
    assert np.array_equal(np.loadtxt(found[0][1], dtype=int, delimiter=",", ndmin=2), a)
    assert not os.path.exists(tmp_path / "exp_run1_s20.csv")
