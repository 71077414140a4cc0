"""The GAN inference programs against the REFERENCE'S OWN TEXT, executed (tests/golden/make_reference_gan_inference.py:
`gan/gan_infer_image_for_shadow.py::main` and `gan/gan_infer_for_shadow.py::main` under stand-ins, with a scripted per-pixel
generator).  CPU only: the conversion runs on the emulation of hypel_denorm_scatter (tests/test_gan_inference.py), which
the GPU tests hold the HIP kernel to bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.common.common_nn_ops import BasicDataSet, calculate_shadow_ratio
from hypelcnn_amd.gan import gan_infer_image_for_shadow as GI
from hypelcnn_amd.gan.gan_train_for_shadow import create_stats
from hypelcnn_amd.gan.wrappers import gan_common as C
from tests.test_gan_inference import DenormEmu, ScriptedGenerator

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "reference_gan_inference.json")))
ARR = np.load(os.path.join(HERE, "golden", "reference_gan_inference.npz"))
CKPT = "/ckpt/model.ckpt-4200"


def _scene(path):
    casi, smap = ARR[f"scene/{path}/casi"], ARR[f"scene/{path}/shadow_map"]
    return BasicDataSet(shadow_creator_dict=None, casi=casi, lidar=None, neighborhood=0, normalize=True), smap


@pytest.mark.parametrize("key", sorted(META["convert"]))
def test_conversion_matches_the_reference_program(key):
    """Per scene dtype x mode x convert_all: the pixels that go through the generator (which, in which order, which
    direction, whether a checkpoint is restored), the raster it writes (dtype and every value) and the file name."""
    path, mode, conv_all = key.rsplit("/", 2)
    mode = "" if mode == "empty" else mode
    convert_all = conv_all == "true"
    m = META["convert"][key]
    ds, smap = _scene(path)
    bands = ds.get_casi_band_count()
    gen = ScriptedGenerator(bands)
    got = GI.convert_scene(ds, smap, GI.parse_mode(mode)[0], convert_all, gen, DenormEmu(), chunk=7)
    want = ARR[f"convert/{key}/raster"]
    assert str(got.dtype) == m["dtype"] == str(want.dtype) and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    fed = np.concatenate(gen.seen) if gen.seen else np.zeros((0, bands), np.float32)
    assert fed.shape[0] == m["n_fed"] and np.array_equal(fed, ARR[f"convert/{key}/fed"])
    assert np.array_equal(GI.select_pixels(smap, GI.parse_mode(mode)[0], convert_all), ARR[f"convert/{key}/fed_pixels"])
    name, is_shadow, _ = GI.parse_mode(mode)
    assert m["direction"] == ["x2y" if is_shadow else "y2x"]
    assert bool(m["restored"]) == (name != "none")  # the product's main restores exactly then
    assert GI.output_name(name, CKPT, convert_all) == m["files"][0]
    assert m["imwrite_kwargs"][0] == {"planarconfig": "contig"}  # chunky, as tiff_io writes it


@pytest.mark.parametrize("key", sorted(META["score"]))
def test_divergences_from_the_recorded_samples(key):
    """The reference's hooks sampled these (x, y) points; the product's samples of them and its statistic
    (create_stats, float64) give the reference's divergences (float32), for every hook the wrapper makes."""
    path, gan_type = key.split("/")
    m = META["score"][key]
    ds, smap = _scene(path)
    ratio = calculate_shadow_ratio(ds.casi, smap, np.logical_not(smap).astype(int))
    points = ARR[f"score/{key}/points"]
    hooks = {"cycle_gan": [("shadowed", False), ("deshadowed", True)], "gan_x2y": [("shadowed", False)],
             "gan_y2x": [("deshadowed", True)]}[gan_type]
    assert sorted(m["best_ratio"]) == sorted(f"best_ratio_{s}.json" for s, _ in hooks)
    assert points.shape == (40 * len(hooks), 2)
    for i, (suffix, fetch_shadows) in enumerate(hooks):
        pts = points[40 * i:40 * (i + 1)]
        assert (smap[pts[:, 1], pts[:, 0]] > 0).all() if fetch_shadows else (smap[pts[:, 1], pts[:, 0]] == 0).all()
        x = C.load_samples_for_testing(ds, pts)
        r = C.adj_shadow_ratio(ratio, fetch_shadows)
        div = create_stats(torch.from_numpy(ScriptedGenerator.g(x)), torch.from_numpy(x), torch.from_numpy(r))[0]
        (it, want), = m["best_ratio"][f"best_ratio_{suffix}.json"]
        assert it == 0 and abs(div - want) <= 2e-5 * abs(want) + 1e-6, (suffix, div, want)


def test_best_ratio_holder_replays_the_reference():
    m = META["best_ratio_holder"]
    h, h2 = C.BestRatioHolder(m["max_size"]), C.BestRatioHolder(m["max_size"])
    for it, d in m["sequence"]:
        h.add_point(np.int64(it), np.float64(d))
    for it, d in m["sequence_2"]:
        h2.add_point(it, d)
    assert [list(p) for p in h.data_holder] == m["holder"]
    assert [list(p) for p in h2.data_holder] == m["holder_2"]
    assert [list(p) for p in C.BestRatioHolder.create_common_iterations(h, h2).data_holder] == m["common"]
    assert json.dumps(h.data_holder) == m["json"]
