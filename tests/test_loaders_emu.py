"""CPU: the four file-backed loaders (GRSS2013, GULFPORT, GULFPORTALT, AVON) against what the reference's own loader
files produced on the same seeded data directory (tests/golden/reference_loaders.*, written by
tests/golden/make_reference_loaders.py): once through the host BasicDataSet and once through DeviceBasicDataSet on the
NumPy emulation of the scene-preparation launches (tests/emu_scene.py)."""
import json
import os
import struct

import numpy as np
import pytest

import tests.emu_scene  # noqa: F401  (registers the scene launches on EmuBackend)
from hypelcnn_amd.common import bmp_io
from hypelcnn_amd.common.common_nn_ops import BasicDataSet, get_loader_from_name
from hypelcnn_amd.loader.DataLoader import LoadingMode
from tests import loader_cases as C
from tests.emu_backend import EmuBackend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NB = C.NEIGHBORHOOD


@pytest.fixture(scope="module")
def gold():
    meta = json.load(open(os.path.join(GOLDEN, "reference_loaders.json")))
    with np.load(os.path.join(GOLDEN, "reference_loaders.npz")) as z:
        return meta, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return C.write_data_dir(str(tmp_path_factory.mktemp("loader_data")))


def cases_of(name):
    if name == "GULFPORTALTDataLoader":
        return [(m.name.lower(), {"_load_mode": m}, True) for m in LoadingMode]
    cases = [("normalized", {}, True), ("raw", {}, False)]
    if name == "AVONDataLoader":
        cases.append(("shcorrected", {"load_shadow_corrected": True}, True))
    return cases


ALL_CASES = [(n, c[0]) for n in C.LOADERS for c in cases_of(n)]


class Pinned:
    """A loader whose scene is prepared on exactly the backend it was given -- None is the host BasicDataSet, on a
    machine with a HIP device too (device_scene.resolve_scene_backend would pick that device otherwise)."""

    def __init__(self, loader):
        self._loader = loader

    def __getattr__(self, name):
        attr = getattr(self._loader, name)
        if not callable(attr):
            return attr

        def pinned(*args, **kwargs):
            import hypelcnn_amd.common.device_scene as D
            real = D.resolve_scene_backend
            D.resolve_scene_backend = lambda backend=None: backend
            try:
                return attr(*args, **kwargs)
            finally:
                D.resolve_scene_backend = real
        return pinned


def load(base, name, case, backend):
    loader = get_loader_from_name(name, base)
    loader.backend = backend
    attrs, normalize = next((a, nrm) for c, a, nrm in cases_of(name) if c == case)
    for k, v in attrs.items():
        setattr(loader, k, v)
    loader = Pinned(loader)
    return loader, loader.load_data(NB, normalize)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def scene_f32(ds, name):
    v = getattr(ds, name)
    return None if v is None else np.asarray(v).astype(np.float32)


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name,case", ALL_CASES)
def test_data_set_matches_reference(gold, base, name, case, path):
    meta, arrays = gold
    backend = EmuBackend() if path == "device" else None
    loader, ds = load(base, name, case, backend)
    key = f"{name}/{case}"
    prim = ds._data_sets[0] if hasattr(ds, "_data_sets") else ds
    assert (type(prim).__name__ == "DeviceBasicDataSet") == (path == "device")
    for what in ("casi_min", "casi_max", "lidar_min", "lidar_max"):
        assert same(getattr(prim, what), arrays[f"{key}/{what}"]), what
    assert ds.get_scene_shape() == meta[key]["scene_shape"] and ds.get_data_shape() == meta[key]["data_shape"]
    assert str(ds.get_unnormalized_casi_dtype()) == meta[key]["casi_dtype"]
    assert (sorted(ds.shadow_creator_dict) if ds.shadow_creator_dict else None) == meta[key]["creators"]
    if path == "device":
        assert prim.downloaded() == [], "shapes, extrema and the shadow ratio must not pull the scene back"
    want = arrays[f"{key}/patches"]
    got = np.stack([np.asarray(prim.get_data_point(x, y)) for x, y in C.POINTS])
    if path == "host":
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
    else:  # a normalised device scene is float32: the golden's values as float32; a raw one keeps the raster's dtype
        want = want if case == "raw" else want.astype(np.float32)
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
    # the whole scene: float64 sum within the summation-order bound n * 2^-53 * sum|x|
    for i, what in enumerate(("casi", "lidar")):
        s = scene_f32(prim, what)
        if s is None:
            continue
        total = np.sum(s, dtype=np.float64)
        bound = s.size * 2.0 ** -53 * np.sum(np.abs(s), dtype=np.float64)
        assert abs(total - arrays[f"{key}/scene_sum"][i]) <= bound
    if "clip_bounds" in "".join(k for k in arrays if k.startswith(key + "/")):
        assert same(prim.clip_bounds, arrays[f"{key}/clip_bounds"])
    shadow = loader.load_shadow_map(NB, ds)
    if meta[key].get("shadow_map", 0) is None:
        assert shadow is None
        return
    assert int(np.asarray(shadow[0], np.int64).sum()) == int(arrays[f"{key}/shadow_map_sum"])
    ratio_ref = arrays[f"{key}/shadow_ratio"]
    if path == "host":
        assert same(shadow[1], ratio_ref)
    else:
        casi = scene_f32(prim, "casi").astype(np.float64)
        on = np.asarray(shadow[0]) != 0
        exact = casi[~on].mean(axis=0) / casi[on].mean(axis=0)
        assert shadow[1].dtype == np.float32
        assert np.all(np.abs(shadow[1].astype(np.float64) - exact) <= 2.0 ** -23 * np.abs(exact))


@pytest.mark.parametrize("name,case", ALL_CASES)
def test_device_scene_equals_host_scene(base, name, case):
    """DeviceBasicDataSet vs BasicDataSet on the same file: the whole prepared scene, bit for bit (as float32: the
    host keeps float64 where NumPy divides integers by an integer scalar)."""
    _, host = load(base, name, case, None)
    _, dev = load(base, name, case, EmuBackend())
    pairs = zip(host._data_sets, dev._data_sets) if hasattr(host, "_data_sets") else [(host, dev)]
    for h, d in pairs:
        assert type(h) is BasicDataSet and type(d).__name__ == "DeviceBasicDataSet"
        for what in ("casi", "lidar"):
            a, b = scene_f32(h, what), scene_f32(d, what)
            assert (a is None) == (b is None)
            if a is not None:
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
        if case == "raw":
            assert d.casi.dtype == h.casi.dtype


def test_percentile_rule_reproduces_numpy():
    from hypelcnn_amd.common.device_scene import percentile_from_ranks, percentile_ranks
    rng = np.random.default_rng(3)
    for trial in range(40):
        h, w, b = rng.integers(1, 40), rng.integers(1, 40), 5
        a = rng.integers(0, 65536 if trial % 2 else 300, (h, w, b)).astype(np.uint16)
        q = [95, 50, 0, 100, 33.3][trial % 5]
        lo, hi, t = percentile_ranks(h * w, q)
        s = np.sort(a.reshape(-1, b), axis=0)
        assert np.array_equal(percentile_from_ranks(s[lo], s[hi], t, np.uint16),
                              np.percentile(a, q, axis=[0, 1]).astype(np.uint16))


def test_avon_clip_changes_every_band(gold, base):
    _, arrays = gold
    from hypelcnn_amd.common.tiff_io import imread
    raw = np.swapaxes(imread(base + "/AVON/0920-1857.georef_cropped.tif")[:, :, C.BLANK:-C.BLANK], 0, 2)
    assert ((raw > arrays["AVONDataLoader/normalized/clip_bounds"]).sum(axis=(0, 1)) > 0).all()


def test_avon_device_path_reads_the_file_in_place(base):
    """the swapped, windowed view reaches the launches as strides over the file's own buffer: no host transpose"""
    be = EmuBackend()
    seen = []
    real = be.k_scene_prepare_f32
    be.k_scene_prepare_f32 = lambda *a: (seen.append(a), real(*a))[1]
    load(base, "AVONDataLoader", "normalized", be)
    src, _, h, w, bands, sy, sx, sb = seen[0][:8]
    assert (h, w, bands) == (C.H, C.W, 12) and (sy, sx, sb) == (1, C.H + 2 * C.BLANK, C.W * (C.H + 2 * C.BLANK))
    assert src.off == C.BLANK * 2 and src.t.numel() == 12 * C.W * (C.H + 2 * C.BLANK) * 2


# ------------------------------------------------------------------------------------------------ targets and splits
def rows_set(rows):
    return {tuple(int(v) for v in r) for r in np.asarray(rows)}


def test_target_rows_match_reference(gold, base):
    _, arrays = gold
    g13 = get_loader_from_name("GRSS2013DataLoader", base)
    for part in ("TR", "VA"):
        assert same(g13.read_targets(f"2013_IEEE_GRSS_DF_Contest_Samples_{part}.tif"),
                    arrays[f"GRSS2013DataLoader/targets/{part}"])
    s = g13.load_samples(1.0, 0)  # no random draw: the contest's split as it is
    assert same(s.training_targets, arrays["GRSS2013DataLoader/samples_ratio0/training"])
    assert same(s.validation_targets, arrays["GRSS2013DataLoader/samples_ratio0/validation"])
    assert s.test_targets.shape == (0, 3)
    for name in ("GULFPORTDataLoader", "GULFPORTALTDataLoader"):
        gp = get_loader_from_name(name, base)
        for f in ("gt", "gt_shadow_corrected"):
            rows = gp.read_targets(f"muulf_{f}.tif")
            assert same(rows, arrays[f"{name}/targets/{f}"])
            assert rows[:, 2].min() == 0 and rows[:, 2].max() == 10
    av = get_loader_from_name("AVONDataLoader", base)
    for no in (1, 2):
        for kind in ("nsh", "sh"):
            rows = av.read_each_target(f"0920-1857.georef_cropped_rgb_with_targets_{no}_{kind}.bmp", target_no=no)
            assert same(rows, arrays[f"AVONDataLoader/targets/{no}_{kind}"])
            assert len(rows) and set(rows[:, 2]) == {no - 1}


def check_split(parts, universe, ratio_of=None):
    seen = [rows_set(p) for p in parts]
    assert sum(len(s) for s in seen) == sum(len(p) for p in parts), "a row occurs twice inside one part"
    for i in range(len(seen)):
        for j in range(i + 1, len(seen)):
            assert not (seen[i] & seen[j])
    assert set().union(*seen) == rows_set(universe)


def test_drawn_splits(gold, base):
    meta, arrays = gold
    g13 = get_loader_from_name("GRSS2013DataLoader", base)
    s = g13.load_samples(1.0, 0.2)
    tr = arrays["GRSS2013DataLoader/targets/TR"]
    check_split([s.training_targets, s.test_targets], tr)
    assert same(s.validation_targets, arrays["GRSS2013DataLoader/targets/VA"])
    assert np.bincount(s.test_targets[:, 2].astype(int), minlength=15).tolist() == \
        meta["loaders"]["GRSS2013DataLoader"]["split_sizes"]["test"]  # random_state 0: the reference's very split

    gp = get_loader_from_name("GULFPORTDataLoader", base)
    s = gp.load_samples(0.7, 0.2)
    gt = arrays["GULFPORTDataLoader/targets/gt"]
    check_split([s.training_targets, s.test_targets, s.validation_targets], gt)
    per_class = np.bincount(gt[:, 2], minlength=11)
    val = np.bincount(s.validation_targets[:, 2].astype(int), minlength=11)
    assert np.all(np.abs(val - 0.3 * per_class) <= 1.0) and len(s.validation_targets) == len(gt) - int(0.7 * len(gt))
    s = gp.load_samples(5, 0)  # per-class training size
    assert np.bincount(s.training_targets[:, 2], minlength=11).tolist() == [5] * 11 and s.test_targets.shape == (0, 3)
    check_split([s.training_targets, s.validation_targets], gt)

    alt = get_loader_from_name("GULFPORTALTDataLoader", base)
    s = alt.load_samples(0.7, 0.2)
    assert s.test_targets.shape == (0, 3)
    smap, none = alt.load_shadow_map(0, None)
    assert none is None
    rows = arrays["GULFPORTALTDataLoader/targets/gt_shadow_corrected"]
    in_shadow = smap[rows[:, 1], rows[:, 0]] != 0
    n_sh = int(in_shadow.sum())
    assert same(s.validation_targets[-n_sh:], rows[in_shadow]), "the shadowed targets close the validation set, in order"
    check_split([s.training_targets, s.validation_targets[:-n_sh]], rows[~in_shadow])

    av = get_loader_from_name("AVONDataLoader", base)
    s = av.load_samples(0.7, 0.2)
    t = {k: arrays[f"AVONDataLoader/targets/{k}"] for k in ("1_nsh", "1_sh", "2_nsh", "2_sh")}
    n_sh = len(t["1_sh"]) + len(t["2_sh"])
    assert same(s.validation_targets[:n_sh], np.vstack([t["1_sh"], t["2_sh"]])), "shadowed targets open the validation set"
    check_split([s.training_targets, s.test_targets, s.validation_targets[n_sh:]], np.vstack([t["1_nsh"], t["2_nsh"]]))
    assert set(s.training_targets[:, 2]) == {0, 1}


# ------------------------------------------------------------------------------------------------ GULFPORTALT
def test_gulfportalt_modes(gold, base):
    meta, arrays = gold
    name = "GULFPORTALTDataLoader"
    assert get_loader_from_name(name, base)._load_mode is LoadingMode.ORIGINAL
    for backend in (None, EmuBackend()):
        _, original = load(base, name, "original", backend)
        for mode in ("shadowed", "deshadowed"):
            _, ds = load(base, name, mode, backend)
            assert same(ds.casi_min, original.casi_min) and same(ds.casi_max, original.casi_max)
            assert not np.array_equal(np.asarray(ds.get_data_point(3, 4)), np.asarray(original.get_data_point(3, 4)))
        _, mixed = load(base, name, "mixed", backend)
        members = mixed._data_sets
        assert [next(j for j, d in enumerate(members) if d is m) for m in members] == meta[f"{name}/mixed"]["members"]
        assert len(members) == 4 and members[1] is members[2] is members[3] and members[0] is not members[1]
        for m in members[1:]:
            assert same(m.casi_min, members[0].casi_min) and same(m.casi_max, members[0].casi_max)
        for i, m in enumerate(members):
            got = np.stack([np.asarray(m.get_data_point(x, y)) for x, y in C.POINTS])
            want = arrays[f"{name}/mixed/member{i}/patches"]
            if backend is None:
                assert got.dtype == want.dtype and np.array_equal(got, want)
            else:
                assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
        hits = set()
        for _ in range(40):
            p = np.asarray(mixed.get_data_point(5, 6))
            match = [i for i in (0, 1) if np.array_equal(p, np.asarray(members[i].get_data_point(5, 6)))]
            assert match, "a MIXED patch is one member's patch"
            hits.add(match[0])
        assert hits == {0, 1}


def test_scene_arrays_mixed_batches(base):
    """SceneArrays over a MultiDataSet: the distinct scenes stay resident, every sample comes from the member drawn
    for it, one gather launch per distinct scene."""
    import torch
    from hypelcnn_amd.common.common_nn_ops import SceneArrays
    be = EmuBackend()
    loader, mixed = load(base, "GULFPORTALTDataLoader", "mixed", be)
    targets = loader.read_targets("muulf_gt.tif")[:50]
    arrays = SceneArrays()
    arrays.feed(mixed, targets, be)
    assert len(arrays.scenes) == 2 and arrays.member_scene == [0, 1, 1, 1]
    assert all(m.downloaded() == [] for m in mixed._data_sets[:2]), "the scenes went from HBM to HBM"
    launches = []
    real = be.k_gather_patches_f32
    be.k_gather_patches_f32 = lambda *a: (launches.append(a), real(*a))[1]
    idx = torch.arange(50)
    out, pts = arrays.gather(idx)
    assert len(launches) == 2 and sorted(int(a[7]) for a in launches) == sorted(
        [int((arrays.last_members == 0).sum()), int((arrays.last_members != 0).sum())])
    assert set(arrays.last_members) == {0, 1, 2, 3}
    for i in range(50):
        member = mixed._data_sets[arrays.last_members[i]]
        want = np.asarray(member.get_data_point(int(targets[i, 0]), int(targets[i, 1])), np.float32)
        assert np.array_equal(out[i].numpy(), want)
    again = SceneArrays()
    again.feed(mixed, targets, be)
    again.gather(idx)
    assert np.array_equal(again.last_members, arrays.last_members), "the member draw is seeded"
    other = SceneArrays()
    other.feed(mixed, targets, be, seed=1234, stream=1)
    other.gather(idx)
    assert not np.array_equal(other.last_members, arrays.last_members), "another iterator kind, another sequence"


def test_gulfport_has_no_shadow_map(base):
    loader = get_loader_from_name("GULFPORTDataLoader", base)
    assert loader.load_shadow_map(NB, None) is None


def test_loader_surface(gold, base):
    meta, arrays = gold
    for name in C.LOADERS:
        loader = get_loader_from_name(name, base)
        info = meta["loaders"][name]
        assert loader.get_model_base_dir() == base + info["model_base_dir"]
        assert [loader.get_class_count().start, loader.get_class_count().stop] == info["class_count"]
        assert same(loader.get_samples_color_list(), arrays[f"{name}/colors"])
        assert same(loader.get_band_measurements(), arrays[f"{name}/bands"])


# ------------------------------------------------------------------------------------------------ bmp_io
def bmp(bits, w, h, palette, rows, top_down=False, compression=0, planes=1):
    """hand-built file: `rows` are the padded lines in FILE order"""
    off = 54 + len(palette)
    data = b"".join(rows)
    return (b"BM" + struct.pack("<IHHI", off + len(data), 0, 0, off) +
            struct.pack("<IiiHHIIiiII", 40, w, -h if top_down else h, planes, bits, compression, len(data), 0, 0,
                        len(palette) // 4, 0) + palette + data)


BW = bytes([0, 0, 0, 0, 255, 255, 255, 0])
GRAY = b"".join(bytes([i, i, i, 0]) for i in range(256))


@pytest.mark.parametrize("top_down", [False, True])
def test_bmp_formats(tmp_path, top_down):
    def read(raw):
        p = tmp_path / "t.bmp"
        p.write_bytes(raw)
        return bmp_io.imread(str(p))

    def order(rows):
        return rows if top_down else rows[::-1]
    # 1 bit, 10 x 2: rows 1010000001 / 0000000011, lines padded to 4 bytes
    img = read(bmp(1, 10, 2, BW, order([bytes([0b10100000, 0b01000000, 0, 0]), bytes([0, 0b11000000, 0, 0])]), top_down))
    assert img.dtype == bool and img.shape == (2, 10)
    assert img.astype(int).tolist() == [[1, 0, 1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 1, 1]]
    # 8 bit gray, 3 x 2
    img = read(bmp(8, 3, 2, GRAY, order([bytes([1, 2, 255, 0]), bytes([9, 0, 7, 0])]), top_down))
    assert img.dtype == np.uint8 and img.tolist() == [[1, 2, 255], [9, 0, 7]]
    # 8 bit with a colour palette: the palette's RGB
    pal = bytes([10, 20, 30, 0, 1, 2, 3, 0])
    img = read(bmp(8, 2, 1, pal, [bytes([1, 0, 0, 0])], top_down))
    assert img.tolist() == [[[3, 2, 1], [30, 20, 10]]]
    # 24 bit, 2 x 2, stored BGR with two bytes of padding per line
    img = read(bmp(24, 2, 2, b"", order([bytes([3, 2, 1, 6, 5, 4, 0, 0]), bytes([9, 8, 7, 12, 11, 10, 0, 0])]), top_down))
    assert img.dtype == np.uint8 and img.tolist() == [[[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [10, 11, 12]]]


def test_bmp_refuses_other_formats(tmp_path):
    def read(raw):
        p = tmp_path / "t.bmp"
        p.write_bytes(raw)
        return bmp_io.imread(str(p))
    line = bytes(8)
    for raw in (bmp(4, 2, 1, bytes(64), [bytes(4)]), bmp(32, 2, 1, b"", [line]), bmp(16, 2, 1, b"", [bytes(4)]),
                bmp(8, 2, 1, GRAY, [bytes(4)], compression=1), bmp(24, 2, 1, b"", [line], planes=2),
                b"PM" + bytes(60), bmp(8, 2, 1, b"", [bytes(4)]),  # 8 bits without room for a palette
                bmp(24, 2, 2, b"", [line])):  # the last one: pixel data cut short
        with pytest.raises(ValueError):
            read(raw)
