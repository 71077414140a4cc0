"""GPU: the two launches of csrc/band_ratio.hip against NumPy itself -- the ratio, its row mask and count bit for bit,
the rank select by value against numpy.sort and identical between two calls -- their refusals, and the validation hook's
band-ratio record on a device generator against the NumPy twins fed the same tensors."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import COLUMN_RANK_WS_WORDS, HypelError, Ref
from tests import band_ratio_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ ratio
def run_ratio(be, num, den, scale, bands, ld_out):
    n = num.shape[0]
    d_num, d_den = be.upload(num), be.upload(den)
    d_scale = None if scale is None else be.upload(scale)
    ratio = be.upload(np.full(n * ld_out, -7.0, np.float32))
    ok = be.upload(np.full(n, 9, np.uint8))
    kept = be.upload(np.full(1, -5, np.int64))  # the call clears it
    be.call("band_ratio_f32", Ref(d_num), num.shape[1], Ref(d_den), den.shape[1], n, bands,
            None if scale is None else Ref(d_scale), Ref(ratio), ld_out, Ref(ok), Ref(kept))
    return ratio.cpu().numpy().reshape(n, ld_out), ok.cpu().numpy(), int(kept.cpu()[0])


@pytest.mark.parametrize("n,bands", K.SHAPES)
def test_ratio_mask_and_count_are_numpys_bits(be, n, bands):
    seen = set()
    for pad, with_scale in ((0, True), (3, False), (5, True)):
        num, den, scale = K.ratio_case(n, bands, pad)
        scale = scale if with_scale else None
        want, want_ok = K.expected_ratio(num, den, scale, bands)
        ld_out = bands + (2 if pad else 0)
        first = run_ratio(be, num, den, scale, bands, ld_out)
        again = run_ratio(be, num, den, scale, bands, ld_out)
        got, ok, kept = first
        assert np.array_equal(bits(got[:, :bands]), bits(want)), (pad, np.argwhere(bits(got[:, :bands]) != bits(want))[:4])
        assert (got[:, bands:] == -7.0).all()  # nothing written between the rows
        assert np.array_equal(ok, want_ok.astype(np.uint8)) and kept == int(want_ok.sum())
        assert np.array_equal(bits(again[0]), bits(got)) and np.array_equal(again[1], ok) and again[2] == kept
        seen |= {bool(v) for v in want_ok}
        if n * bands > 4000:
            flat = want.reshape(-1)
            assert np.isnan(flat).any() and np.isinf(flat).any() and (flat < 0).any()
            assert ((flat != 0) & (np.abs(flat) < np.float32(1.2e-38))).any()  # denormal results too
    if n > 8:
        assert seen == {True, False}


# ------------------------------------------------------------------------------------------------ rank select
def run_select(be, d_x, ld, n, bands, d_ok, m, ranks, ws):
    out = be.upload(np.full(len(ranks) * bands, np.nan, np.float32))
    be.call("column_rank_select_f32", Ref(d_x), ld, n, bands, None if d_ok is None else Ref(d_ok), m,
            Ref(torch.tensor(ranks, dtype=torch.int64)), len(ranks), Ref(out), Ref(ws))
    return out.cpu().numpy().reshape(len(ranks), bands)


@pytest.mark.parametrize("n,bands", K.SHAPES)
def test_rank_select_is_numpys_sort(be, n, bands):
    ws = be.empty(bands * COLUMN_RANK_WS_WORDS, torch.int32)  # reused dirty: the call clears it
    # every data set at every row stride: no padding, one that rules 16-byte loads out, and the one that makes the
    # stride a multiple of 4 floats (float4 loads, with whole and partial groups of 4 columns)
    pads = sorted({0, 3, (-bands) % 4, (-bands) % 4 + 4})
    assert any((bands + p) % 4 == 0 for p in pads) and any((bands + p) % 4 for p in pads)
    for at, kind in enumerate(K.DATA_SETS):
        for pad in pads:
            for m in K.kept_counts(n):
                x, ok = K.select_case(kind, n, bands, m, pad)
                d_x = be.upload(x)
                d_ok = None if (m == n and at < 3) else be.upload(ok)  # the null mask: all rows
                for count in K.RANK_COUNTS:
                    ranks = K.ranks_for(m, count)
                    want = K.expected_select(x, ok, bands, ranks)
                    got = run_select(be, d_x, bands + pad, n, bands, d_ok, m, ranks, ws)
                    again = run_select(be, d_x, bands + pad, n, bands, d_ok, m, ranks, ws)
                    assert np.array_equal(got, want), (kind, pad, m, count, np.argwhere(got != want)[:4])  # -0 == +0
                    assert np.array_equal(bits(got), bits(again)), (kind, pad, m, count)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_named_and_launch_nothing(be):
    n, bands = 5, 3
    x = be.upload(np.arange(n * bands, dtype=np.float32))
    ok = be.upload(np.ones(n, np.uint8))
    out = be.upload(np.full(8 * bands, -3.0, np.float32))
    ws = be.upload(np.full(bands * COLUMN_RANK_WS_WORDS, 77, np.int32))
    kept = be.upload(np.full(1, 41, np.int64))
    r = lambda *v: Ref(torch.tensor(v, dtype=torch.int64))  # noqa: E731
    X, OK, OUT, WS, KEPT = Ref(x), Ref(ok), Ref(out), Ref(ws), Ref(kept)
    select = [
        (X, bands, 0, bands, OK, 0, r(0), 1, OUT, WS),            # n < 1
        (X, bands, n, 0, OK, n, r(0), 1, OUT, WS),                # bands < 1
        (X, bands, 1 << 31, bands, OK, n, r(0), 1, OUT, WS),      # n >= 2^31
        (X, bands, n, bands, OK, n, r(0), 0, OUT, WS),            # n_ranks out of range
        (X, bands, n, bands, OK, n, r(0, 1, 2, 3, 4, 0, 1, 2, 3), 9, OUT, WS),
        (X, bands, n, bands, OK, 4, r(0, 4), 2, OUT, WS),         # a rank outside the kept count
        (X, bands, n, bands, OK, n, r(-1), 1, OUT, WS),
        (X, bands, n, bands, None, 4, r(0), 1, OUT, WS),          # no mask: every row is kept
        (X, bands - 1, n, bands, OK, n, r(0), 1, OUT, WS),        # row stride below the width
        (X, 65537, n, 65537, OK, n, r(0), 1, OUT, WS),            # more columns than one call takes
    ]
    ratio = [
        (X, bands, X, bands, 0, bands, None, OUT, bands, OK, KEPT),
        (X, bands, X, bands, n, 0, None, OUT, bands, OK, KEPT),
        (X, bands, X, bands, 1 << 31, bands, None, OUT, bands, OK, KEPT),
        (X, bands, X, bands - 1, n, bands, None, OUT, bands, OK, KEPT),
        (X, bands, X, bands, n, bands, None, None, bands, OK, KEPT),
    ]
    for name, calls in (("column_rank_select_f32", select), ("band_ratio_f32", ratio)):
        for args in calls:
            with pytest.raises(HypelError, match=f"hypel_{name}.*invalid argument"):
                be.call(name, *args)
    be.synchronize()
    assert (out.cpu().numpy() == -3.0).all() and (ws.cpu().numpy() == 77).all() and int(kept.cpu()[0]) == 41
    assert (ok.cpu().numpy() == 1).all()
    # and the same buffers still serve a good call
    got = run_select(be, x, bands, n, bands, ok, n, [4, 0], ws)
    assert np.array_equal(got, np.float32([[12, 13, 14], [0, 1, 2]]))


# ------------------------------------------------------------------------------------------------ the hook
def test_hook_record_on_a_device_generator_is_the_twins(be, tmp_path):
    import tests.emu_band_ratio  # noqa: F401 -- the NumPy twins, on EmuBackend
    from hypelcnn_amd.common import band_ratio as BR
    from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict
    from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
    from tests.emu_backend import EmuBackend
    loader = SyntheticDataLoader("gulfport:h=12:w=14:bands=16:classes=3:samples=0.6")
    ds = loader.load_data(0, True)
    smap, shadow_ratio = loader.load_shadow_map(0, ds)
    hook = get_infer_wrapper_dict()["gan_x2y"].create_inference_hook(ds, loader, str(tmp_path), 0, smap, shadow_ratio,
                                                                     0, 64, backend=be)
    sess = hook.ctx.session()
    rng = np.random.default_rng(8)
    for name, value in sess.state_dict().items():  # a generator that is not the zero of a fresh initialisation
        if name in sess.store.vars and np.asarray(value).dtype.kind == "f":
            sess.set_variable(name, (rng.standard_normal(np.shape(value)) * 0.3).astype(np.float32))
    hook.band_ratio_stats = True
    hook.after_run(3)
    got = json.load(open(tmp_path / "band_ratio_shadowed_3.json"))
    x = hook._data_sample_list
    ct = sess.compile_phase(hook.ctx.tower, 64, outputs=[hook._infer_model], key="validate_shadowed")
    ct.set_input(hook._input_tensor.name, torch.as_tensor(x).to(be.device))
    ct.forward()
    gen = ct.value(hook._infer_model, copy=True).cpu().numpy()
    assert gen.shape == (64, 16) and np.abs(gen).max() > 1e-3
    twin = BR.write_band_ratio(str(tmp_path / "twin"), "band_ratio_shadowed", 3, loader.get_band_measurements(),
                               BR.band_ratio_stats(EmuBackend(), gen, x, np.asarray(shadow_ratio, np.float32)),
                               "p50", "p10", "p90")
    assert got.keys() == twin.keys() and got["kept"] > 0
    for key in ("step", "bands", "samples", "kept", "p10", "p50", "p90"):
        assert got[key] == twin[key], key
    for key in ("mean", "std"):  # float64 moments of 64 rows, summed in another order
        np.testing.assert_allclose(got[key], twin[key], rtol=1e-9)
    assert got == hook.last_band_ratio
    try:
        import matplotlib.figure  # noqa: F401
        assert open(tmp_path / "band_ratio_shadowed_3.pdf", "rb").read(4) == b"%PDF"
    except ImportError:
        assert not os.path.exists(tmp_path / "band_ratio_shadowed_3.pdf")
