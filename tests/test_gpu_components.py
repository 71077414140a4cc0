"""GPU: the shadow-region launches of csrc/components.hip against the flood-fill oracle and the known answers of
tests/component_cases.py, every launch twice with identical results, the correction against NumPy's float32 expression
bit for bit, and reveal_shadow_targets on the device against the same run on the NumPy emulation, file by file.
Everything is compared exactly.  (A status word other than HYPEL_COMPONENTS_OK makes the wrapper raise.)"""
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import COMPONENTS_OK, Ref
from hypelcnn_amd.common import device_components as dc
from tests import component_cases as C
from tests.test_components_emu import (check_reveal_outputs, correction_sources, host, numpy_correction, run_labelling,
                                       run_votes, write_gulfport)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("name", list(C.MASKS))
def test_labelling_and_compaction(be, name):
    mask, root, comp, n, size = C.mask_case(name)
    got_root, got_comp, got_n = run_labelling(be, mask)
    assert got_n == n
    assert np.array_equal(host(got_root, mask.shape), root) and np.array_equal(host(got_comp, mask.shape), comp)
    again_root, again_comp, again_n = run_labelling(be, mask)
    assert again_n == n and same(again_root, got_root) and same(again_comp, got_comp)
    targets = np.where(mask != 0, C.SHADOW, 1).astype(np.uint8)
    _, got_size, _, _ = run_votes(be, targets, got_comp, got_n)
    assert np.array_equal(host(got_size), size)


def test_status_word_is_cleared_and_stays_clean(be):
    mask = C.mask_case("spiral_97x131")[0]
    h, w = mask.shape
    root, ws = be.empty(h * w, torch.int32), be.empty(h * w, torch.int32)
    status = be.upload(np.array([77], np.int32))  # the call clears it
    be.call("components_label_u8", Ref(be.upload(mask)), h, w, Ref(root), Ref(ws), Ref(status))
    assert int(status.cpu()[0]) == COMPONENTS_OK
    assert np.array_equal(host(root, mask.shape), C.mask_case("spiral_97x131")[1])


@pytest.mark.parametrize("name", C.RANDOM_WITH_TARGETS)
def test_votes_on_random_masks(be, name):
    mask, _, _, _, size = C.mask_case(name)
    targets, votes, winner, out, out_plus = C.random_vote_case(name)
    _, comp, n = run_labelling(be, mask)
    got = run_votes(be, targets, comp, n)
    assert np.array_equal(host(got[0], votes.shape), votes) and np.array_equal(host(got[1]), size)
    assert np.array_equal(host(got[2]), winner) and np.array_equal(host(got[3], mask.shape), out)
    again = run_votes(be, targets, comp, n)
    assert all(same(a, b) for a, b in zip(again, got))
    assert np.array_equal(host(run_votes(be, targets, comp, n, plus_one=True)[3], mask.shape), out_plus)


@pytest.mark.parametrize("name", list(C.KNOWN))
def test_known_answers(be, name):
    case = C.known_case(name)
    targets = case["targets"]
    _, comp, n = run_labelling(be, (targets == C.SHADOW).astype(np.uint8))
    votes, _, winner, out = run_votes(be, targets, comp, n)
    assert host(winner).tolist() == case["winners"]
    votes = host(votes, (n, C.N_CLASSES))
    for (blob, cls), count in case["votes"].items():
        assert votes[blob, cls] == count
    assert np.array_equal(host(out, targets.shape), case["out"])
    assert np.array_equal(host(run_votes(be, targets, comp, n, plus_one=True)[3], targets.shape), case["out_plus_one"])


@pytest.mark.parametrize("kind", list(correction_sources()))
def test_correction_is_numpys_float32_expression(be, kind):
    src = correction_sources()[kind]
    h, w, bands = src.shape
    rng = np.random.default_rng(5)
    smap = (rng.random((h, w)) < 0.4).astype(np.uint8)
    ratio = (1 + rng.random(bands) * 4).astype(np.float32)
    map_d = be.upload(smap)
    got = dc.shadow_correct(be, src, map_d, ratio)
    want = numpy_correction(src, smap, ratio)
    assert np.array_equal(host(got, src.shape).view(np.uint32), want.view(np.uint32))
    assert same(dc.shadow_correct(be, src, map_d, ratio), got)


def test_reveal_shadow_targets_on_the_device_writes_the_emulations_files(be, tmp_path):
    from hypelcnn_amd.utilities import reveal_shadow_targets
    from tests.emu_backend import EmuBackend
    results = {}
    for name, backend in (("device", be), ("emulation", EmuBackend())):
        base = str(tmp_path / name)
        gt, hsi, blobs = write_gulfport(base)
        results[name] = reveal_shadow_targets.main(["--loader_name", "GULFPORTDataLoader", "--path", base,
                                                    "--output_path", base + "/GULFPORT"], backend=backend)
        check_reveal_outputs(base, results[name], gt, hsi, blobs)
    for name in ("muulf_shadow_map.tif", "muulf_hsi_shadow_corrected.tif", "muulf_gt_shadow_corrected.tif",
                 "targets.tif", "targets_shadow_corrected.tif"):
        files = [open(os.path.join(str(tmp_path / which), "GULFPORT", name), "rb").read()
                 for which in ("device", "emulation")]
        assert len(files[0]) > 0 and files[0] == files[1], name
    for key in ("ratio", "winners", "sizes"):
        assert np.array_equal(results["device"][key], results["emulation"][key]), key
