"""-m gpu: GAN shadow inference on the MI355X.  hypel_denorm_scatter bit for bit against its specification
(tests/test_gan_inference.py::DenormEmu), whole-scene conversion against the float64 oracle generator
(oracle/gan.py, oracle/models.py) on a small and on the GRSS2013-size scene, and checkpoint scoring."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import OUT_DTYPES, Ref
from hypelcnn_amd.gan import gan_infer_for_shadow as GS
from hypelcnn_amd.gan import gan_infer_image_for_shadow as GI
from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict
from hypelcnn_amd.gan.wrappers import gan_common as C
from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
from oracle import gan as OG
from oracle import models as OM
from oracle import ops as OO
from tests.test_gan_inference import EDGES, DenormEmu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16, np.uint8])
@pytest.mark.parametrize("bands", [5, 48, 144, 360])
@pytest.mark.parametrize("layout", ["identity", "rows", "padded_rows", "padded_both"])
def test_denorm_scatter_bit_exact(hip, dtype, bands, layout):
    """padded_both: both row strides a multiple of 4 above the band count, so the four-band path runs and a bands % 4
    remainder (bands = 5) goes through its tail."""
    rng = np.random.default_rng(bands + 3 * OUT_DTYPES[np.dtype(dtype)])
    n, total = 1000, 1300
    pad4 = (bands + 3) // 4 * 4 + 4
    ld_src = {"padded_rows": bands + 3, "padded_both": pad4}.get(layout, bands)
    ld_out = pad4 if layout == "padded_both" else bands
    src = (rng.standard_normal((n, ld_src)) * 1.3).astype(np.float32)
    flat = src[:40, :bands].reshape(-1)
    flat[: EDGES.size] = EDGES
    src[:40, :bands] = flat.reshape(40, bands)
    if dtype == np.float32:
        scale, offset = rng.random(bands).astype(np.float32) * 3000, rng.random(bands).astype(np.float32) * 500
    else:
        info = np.iinfo(dtype)
        scale = rng.integers(1, info.max, bands).astype(np.float32)
        offset = rng.integers(max(info.min, 0), info.max // 2, bands).astype(np.float32)
    scale[:3], offset[:3] = 1, 0  # the edge values land unscaled in the first bands
    rows = None if layout == "identity" else rng.permutation(total)[:n].astype(np.int64)
    item = np.dtype(dtype).itemsize
    results = []
    for be in (hip, DenormEmu()):
        out = torch.full((total * ld_out * item,), 0xAB, dtype=torch.uint8, device=be.device)
        be.call("denorm_scatter", Ref(be.upload(src)), ld_src, None if rows is None else Ref(be.upload(rows)), n, bands,
                Ref(be.upload(scale)), Ref(be.upload(offset)), OUT_DTYPES[np.dtype(dtype)], Ref(out), ld_out)
        be.synchronize()
        results.append(out.cpu().numpy())
    assert np.array_equal(results[0], results[1])
    written = np.zeros((total, ld_out * item), bool)
    written[np.arange(n) if rows is None else rows, :bands * item] = True
    assert (results[0].reshape(total, ld_out * item)[~written] == 0xAB).all()


def _generator_params(bands, seed=5):
    return U32(OG.init_gan_params("cycle_gan", bands, np.random.default_rng(seed), dtype=np.float64,
                                  zero_generator=False))


def U32(params):
    return {k: v.astype(np.float32).astype(np.float64) for k, v in params.items()}


def _oracle_g(params, x, is_shadow):
    prefix = "Model/ModelX2Y/Generator/" if is_shadow else "Model/ModelY2X/Generator/"
    n, b = x.shape
    return OM.generator_forward(OM.Ctx(params, False), OO.Var(x.astype(np.float64).reshape(n, 1, 1, b)),
                                prefix=prefix).v.reshape(n, b)


def _convert(hip, loader, params, mode, convert_all, chunk):
    ds = loader.load_data(0, True)
    smap, _ = loader.load_shadow_map(0, ds)
    _, is_shadow, _ = GI.parse_mode(mode)
    gen = GI.GeneratorChunks(get_infer_wrapper_dict()["cycle_gan"], is_shadow, ds.get_casi_band_count(), hip)
    gen.load(params)
    timings = {}
    img = GI.convert_scene(ds, smap, mode, convert_all, gen, hip, chunk=chunk, timings=timings)
    return ds, smap, is_shadow, img, timings


def _check_against_oracle(casi, flat, casi_max, casi_min, is_shadow, params, rows, converted_mask):
    """casi [P, bands] normalised input, flat [P, bands] converted raster; rows: the converted pixels."""
    dtype = flat.dtype
    passthrough = ((casi * casi_max) + casi_min).astype(dtype)
    keep = ~converted_mask
    assert np.array_equal(flat[keep].view(np.uint8), passthrough[keep].view(np.uint8)), "pass-through pixels"
    if rows.size == 0:
        return 0.0
    g64 = _oracle_g(params, casi[rows], is_shadow)
    scale = np.asarray(casi_max, np.float64)
    offset = np.asarray(casi_min, np.float64)
    if dtype == np.float32:
        got_g = (flat[rows].astype(np.float64) - offset) / scale
        err = np.abs(got_g - g64).max()
        assert err < 5e-5, err  # the generator's output in [-1, 1]: the GAN tolerance of test_gpu_gan.py
        return err
    want = np.trunc(g64 * scale + offset).astype(np.int64)
    d = (flat[rows].astype(np.int64) - want) % (1 << (8 * dtype.itemsize))
    assert np.isin(d, [0, 1, (1 << (8 * dtype.itemsize)) - 1]).all(), np.unique(d)
    return float((d != 0).mean())


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
@pytest.mark.parametrize("mode,convert_all", [("shadow", False), ("deshadow", False), ("none", False),
                                              ("shadow", True), ("deshadow", True), ("none", True)])
def test_small_scene_against_oracle(hip, dtype, mode, convert_all):
    scene = "grss2013:h=37:w=45" + ("" if dtype == "float32" else f":dtype={dtype}")
    loader = SyntheticDataLoader(scene)
    params = _generator_params(144)
    ds, smap, is_shadow, img, _ = _convert(hip, loader, params, mode, convert_all, chunk=500)
    assert img.dtype == np.dtype(dtype) and img.shape == (37, 45, 144)
    rows = GI.select_pixels(smap, mode, convert_all)
    mask = np.zeros(smap.size, bool)
    mask[rows] = True
    _check_against_oracle(ds.casi.reshape(-1, 144), img.reshape(-1, 144), ds.casi_max, ds.casi_min, is_shadow, params,
                          rows, mask)


def test_full_size_scene_chunking_is_bit_identical(hip, tmp_path):
    """The GRSS2013 geometry (349 x 1905 x 144, uint16), every pixel through X2Y, at two chunk sizes with different
    tails: the rasters are identical; a 2 000-pixel sample agrees with the float64 oracle within one LSB."""
    loader = SyntheticDataLoader("grss2013:h=349:w=1905:dtype=uint16")
    params = _generator_params(144, seed=11)
    ds, smap, is_shadow, img_a, t_a = _convert(hip, loader, params, "shadow", True, chunk=65536)
    _, _, _, img_b, t_b = _convert(hip, loader, params, "shadow", True, chunk=50000)
    assert img_a.shape == (349, 1905, 144) and img_a.dtype == np.uint16
    assert np.array_equal(img_a, img_b)
    rows = np.sort(np.random.default_rng(0).choice(smap.size, 2000, replace=False))
    off_by_one = _check_against_oracle(ds.casi.reshape(-1, 144)[rows], img_a.reshape(-1, 144)[rows], ds.casi_max,
                                       ds.casi_min, is_shadow, params, np.arange(2000), np.ones(2000, bool))
    print("\nfull scene:", json.dumps({"chunk_65536": t_a, "chunk_50000": t_b, "lsb_off_share": off_by_one}))


@pytest.mark.parametrize("gan_type", ["cycle_gan", "gan_x2y"])
def test_scoring_against_oracle(hip, tmp_path, gan_type):
    scene = "grss2013:h=40:w=50"
    bands = 144
    params = U32(OG.init_gan_params(gan_type, bands, np.random.default_rng(4), dtype=np.float64, zero_generator=False))
    ckpt = str(tmp_path / "model.ckpt-3.npz")
    np.savez(ckpt, **{k.replace("/", "|"): v.astype(np.float32) for k, v in params.items()})
    divs = GS.main(["--loader_name", "SyntheticDataLoader", "--path", scene, "--base_log_path", ckpt,
                    "--number_of_samples", "600", "--gan_type", gan_type], backend=hip)
    loader = SyntheticDataLoader(scene)
    ds = loader.load_data(0, True)
    smap, ratio = loader.load_shadow_map(0, ds)
    from hypelcnn_amd.gan.gan_train_for_shadow import create_stats
    cases = [(False, ratio, "Model/ModelX2Y/Generator/"), (True, 1. / ratio, "Model/ModelY2X/Generator/")] \
        if gan_type == "cycle_gan" else [(False, ratio, "Model/Generator/")]
    assert len(divs) == len(cases)
    for got, (fetch_shadows, r, prefix) in zip(divs, cases):
        idx = C.sample_indices_for_testing(600, 0, smap, fetch_shadows, np.random.default_rng(1234))
        x = C.load_samples_for_testing(ds, idx).astype(np.float64)
        g = OM.generator_forward(OM.Ctx(params, False), OO.Var(x.reshape(-1, 1, 1, bands)), prefix=prefix).v
        want = create_stats(torch.from_numpy(g.reshape(-1, bands)), torch.from_numpy(x),
                            torch.from_numpy(np.asarray(r, np.float64)))[0]
        assert abs(got - want) <= 1e-3 * abs(want) + 1e-6, (gan_type, fetch_shadows, got, want)
    assert os.path.exists(str(tmp_path / "model.ckpt-3" / "best_ratio_shadowed.json"))
