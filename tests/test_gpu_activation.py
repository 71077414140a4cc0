"""GPU: the activation launches of csrc/activation.hip against the float64 numpy.histogram reference of
tests/activation_cases.py -- bin counts, `outside`, the finite and non-finite counts, minimum and maximum all exactly
equal, with sentinel-filled gaps around and between the rows of every view -- accumulation over calls and views, the
contention cases, every launch twice with identical results; common/device_activation.ActivationTaps and
utilities/nn_layer_activation_graph on the device with the tiny HYPELCNN of tests/test_activation_emu.py, against
numpy.histogram over the taps fetched from the same forwards."""
import numpy as np
import pytest

from tests import activation_cases as A
from tests import test_activation_emu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory, be):
    return T.write_checkpoint(tmp_path_factory.mktemp("activation"), be)


@pytest.mark.parametrize("name", A.NAMES)
def test_view_cases(be, name):
    c = A.case(name)
    got = A.run_case(be, c)
    A.check_case(got, c)
    again = A.run_case(be, c)
    assert np.array_equal(again.pop("counts"), got.pop("counts")) and again == got


@pytest.mark.parametrize("kind", ["one", "two"])
def test_contention(be, kind):
    T.check_contention(be, kind)


def test_accumulation(be):
    T.check_accumulation(be)


def test_taps_of_one_forward(be, checkpoint):
    T.check_taps_of_one_forward(be, *checkpoint)


@pytest.mark.parametrize("domain", ["controlled", "sample"])
def test_tool_end_to_end(be, checkpoint, tmp_path, capsys, domain):
    T.check_tool(be, *checkpoint, tmp_path / "out", domain, capsys)
