"""CPU: ABI 8 -- the grid-search entry points are declared and exported (their binding: tests/test_abi.py), and
hypel_svm_job_t's numpy dtype has the header's layout (a hypel_svm_pair_t, then k_off and c)."""
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_svm_kernel_planes_f32", "hypel_svm_smo_grid", "hypel_svm_scatter_coef_f32", "hypel_svm_vote_score")


def test_version_8_and_new_symbols(lib):  # noqa: F811
    from hypelcnn_amd import backend
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert header == backend.ABI_VERSION == lib.hypel_version() == 8
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name)


def test_job_record_layout():
    from hypelcnn_amd.backend import SVM_JOB_DTYPE, SVM_PAIR_DTYPE
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} hypel_svm_job_t;", src).group(1)
    fields = [f.split()[-1] for f in body.split(";") if f.strip()]
    assert fields == list(SVM_JOB_DTYPE.names) == list(SVM_PAIR_DTYPE.names) + ["k_off", "c"]
    assert SVM_JOB_DTYPE.itemsize == 40 and SVM_PAIR_DTYPE.itemsize == 24
    for name in SVM_PAIR_DTYPE.names:  # a job starts with its pair, field for field
        assert SVM_JOB_DTYPE.fields[name] == SVM_PAIR_DTYPE.fields[name]
    assert SVM_JOB_DTYPE.fields["k_off"][1] == 24 and SVM_JOB_DTYPE.fields["c"][1] == 32
    assert SVM_JOB_DTYPE.fields["c"][0].kind == "f" and SVM_JOB_DTYPE.fields["k_off"][0].itemsize == 8
