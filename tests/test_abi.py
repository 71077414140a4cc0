"""CPU: the C-ABI library loads and exports every symbol include/hypel.h declares, and every one of them is bound with
the argument and return types the header declares -- read here by this file's OWN regular expressions, independent of
the package's reader (hypelcnn_amd/abi.py), which is what the binding is built from (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypel.h")

_KINDS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
          "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int, "hypel_stream_t": ctypes.c_void_p}


def _declared():
    """name -> (return kind, [(C type words, parameter name, kind)]): pointers are c_void_p (a returned `const char*`
    c_char_p), scalars the ctypes of the header's width."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"^[ \t]*(const char\*|\w+)\s+(hypel_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S | re.M):
        args = m.group(3).strip()
        params = []
        for a in [] if args in ("", "void") else args.split(","):
            words = a.replace("*", "* ").split()
            ctype = [w for w in words[:-1] if w != "const"]
            params.append((" ".join(ctype), words[-1], ctypes.c_void_p if "*" in a else _KINDS[ctype[0]]))
        out[m.group(2)] = (ctypes.c_char_p if "*" in m.group(1) else _KINDS[m.group(1)], params)
    return out


@pytest.fixture(scope="module")
def lib():
    from hypelcnn_amd import backend
    if not os.path.exists(backend.LIB_PATH):
        backend.build_library()
    return backend.load_library()


def test_every_declared_symbol_is_exported(lib):
    decl = _declared()
    assert len(decl) >= 30
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in hypel.h but not exported"
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    from hypelcnn_amd import backend
    assert lib.hypel_version() == header == backend.ABI_VERSION
    assert lib.hypel_last_error() is not None


def test_signature_table_matches_header(lib):
    """Every declared function: exported, bound, argtypes and restype as the header declares them, the stream last."""
    from hypelcnn_amd import backend
    decl = _declared()
    assert len(decl) >= 120
    launches = {}
    for name, (ret, params) in decl.items():
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} declared in hypel.h but not exported"
        assert fn.argtypes is not None, f"{name} is not bound"
        kinds = [k for _, _, k in params]
        assert list(fn.argtypes) == kinds, f"{name}: bound {list(fn.argtypes)}, header {[(t, n) for t, n, _ in params]}"
        assert fn.restype is ret, f"{name}: bound to return {fn.restype}, header {ret}"
        streams = [i for i, (t, _, _) in enumerate(params) if t == "hypel_stream_t"]
        if name == "hypel_graph_end_capture":
            # the one prototype whose stream is followed by an out-parameter (the captured graph): not a launch
            assert [(t, n) for t, n, _ in params] == [("hypel_stream_t", "stream"), ("void* *", "graph_exec_out")]
        elif streams:
            assert streams == [len(params) - 1] and params[-1][1] == "stream", f"{name}: the stream is not last"
            if not name.startswith("hypel_graph_"):
                launches[name[len("hypel_"):]] = kinds[:-1]
    # the launch table tests and tools index: short name -> argument kinds without the stream
    assert backend.SIGNATURES == launches and len(launches) >= 100


def test_package_reader_finds_every_prototype():
    from hypelcnn_amd import abi
    decl = _declared()
    assert len(abi.FUNCTIONS) == len(decl) and set(abi.FUNCTIONS) == set(decl)
    for name, (_, params) in decl.items():
        assert [p for p, _ in abi.FUNCTIONS[name][1]] == [n for _, n, _ in params], name


@pytest.mark.parametrize("text,what", [
    ("int hypel_f(const float* x,\n            size_t n,\n            hypel_stream_t stream);\n", "size_t"),  # unknown type
    ("int hypel_f(const float* x,\n            int64_t,\n            hypel_stream_t stream);\n", "unnamed"),
    ("int hypel_f(const float*,\n            int64_t n,\n            hypel_stream_t stream);\n", "unnamed"),
    ("int hypel_f(const float* x,\n            int64_t n,\n            hypel_stream_t);\n", "unnamed"),
    ("int hypel_f(int64_t n)\nint hypel_g(void);\n", "hypel_f"),  # (a prototype the reader cannot consume)
    ("typedef struct { int64_t a; short b; } hypel_x_t;\n", "short b"),
])
def test_package_reader_refuses_what_it_does_not_understand(text, what):
    from hypelcnn_amd import abi
    with pytest.raises(abi.HypelError, match=what):
        abi.parse(text)


def test_arg_index_names_the_header_parameter():
    from hypelcnn_amd import backend
    assert backend.arg_index("bn_act_bwd_reduce", "partial") == 14
    assert backend.arg_index("gan_generator_bwd_apps", "pw") == 17 and backend.arg_index("nce_loss", "ws") == 17
    assert backend.arg_index("_allgather", "dst") == 2
    with pytest.raises(backend.HypelError, match=r"no parameter 'sums'.*\(partial, n_chunks, chunk_rows, rows, c, eps"):
        backend.arg_index("bn_finalize", "sums")


def test_table_struct_layouts_match_header():
    from hypelcnn_amd.backend import GROUP_DTYPE, LOSS_TERM_DTYPE, SEG_DTYPE, TILE_DTYPE
    assert LOSS_TERM_DTYPE.itemsize == 104 and LOSS_TERM_DTYPE.fields["mode"][1] == 72 and LOSS_TERM_DTYPE.fields["slot"][1] == 100
    assert SEG_DTYPE.itemsize == 24 and GROUP_DTYPE.itemsize == 24 and TILE_DTYPE.itemsize == 56
    assert TILE_DTYPE.fields["n"][1] == 52  # hypel_tile_t.n (ABI 4) sits where `reserved` was
    from hypelcnn_amd.backend import COPY_BLOCK_DTYPE
    assert COPY_BLOCK_DTYPE.itemsize == 40 and COPY_BLOCK_DTYPE.fields["rows"][1] == 16
    assert SEG_DTYPE.fields["b_off"][1] == 8 and SEG_DTYPE.fields["k"][1] == 16
    assert GROUP_DTYPE.fields["seg_begin"][1] == 8 and GROUP_DTYPE.fields["rows"][1] == 16
    from hypelcnn_amd.backend import (FOREST_NODE_DTYPE, MTILE_DTYPE, REDUCE_ENTRY_DTYPE, SVM_JOB_DTYPE, SVM_PAIR_DTYPE,
                                      TIFF_SEG_DTYPE)
    assert MTILE_DTYPE.itemsize == 72 and MTILE_DTYPE.fields["flags"][1] == 52
    assert REDUCE_ENTRY_DTYPE.itemsize == 40 and REDUCE_ENTRY_DTYPE.fields["n_splits"][1] == 32
    assert SVM_PAIR_DTYPE.itemsize == 24 and SVM_PAIR_DTYPE.fields["out_off"][1] == 16
    assert SVM_JOB_DTYPE.itemsize == 40 and SVM_JOB_DTYPE.fields["k_off"][1] == 24
    assert TIFF_SEG_DTYPE.itemsize == 32 and TIFF_SEG_DTYPE.fields["dst_off"][1] == 16
    assert FOREST_NODE_DTYPE.itemsize == 16 and FOREST_NODE_DTYPE.fields["left"][1] == 8
    from hypelcnn_amd import abi
    assert len(abi.STRUCTS) == 11  # every struct of the header is covered above


def test_no_cpu_fallback_without_gpu():
    import torch
    from hypelcnn_amd.backend import HipBackend, HypelError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(HypelError):
        HipBackend()


def test_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "hypelcnn_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", txt, flags=re.M), os.path.join(dp, f)
