"""CPU: the three forest-diagnostics entry points are declared in include/hypel.h beside the other hypel_forest_*, exported
by the library and bound from the header, add no struct, and refuse null pointers, sizes outside their contract, node
records off their 16-byte alignment and a grid above 2^31 - 1 blocks with a message before anything is launched.  The ABI
version is still 8: new symbols only."""
import ctypes

from hypelcnn_amd import abi
from tests.test_abi import _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_forest_oob_rows", "hypel_forest_permuted_hits", "hypel_forest_importances_f64")


def test_new_symbols_are_declared_bound_and_exported(lib):  # noqa: F811
    from hypelcnn_amd import backend
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name) and name[len("hypel_"):] in backend.SIGNATURES
    assert lib.hypel_version() == backend.ABI_VERSION == 8
    assert abi.const("HYPEL_FOREST_IMPORTANCE_WINDOW") == 4096  # 12 B of LDS a column: 48 KB


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * (4096 + 16))()
    p = (ctypes.addressof(buf) + 15) // 16 * 16  # never dereferenced: every call below fails its argument check first

    def oob(**kw):
        a = dict(x=p, ld=4, n=8, f=4, tree_off=p, n_trees=1, nodes=p, n_nodes=3, leaf_value=p, n_leaves=2, n_classes=3,
                 class_labels=None, weight=p, ldw=8, out=p, proba=p, votes=p)
        a.update(kw)
        return tuple(a.values())

    def hits(**kw):
        a = dict(x=p, ld=4, n=8, f=4, tree_off=p, n_trees=1, nodes=p, n_nodes=3, leaf_value=p, n_leaves=2, n_classes=3,
                 y=p, partner=p, n_repeats=2, group_mod=4, g0=0, n_groups=4, hits=p)
        a.update(kw)
        return tuple(a.values())

    def imp(**kw):
        a = dict(nodes=p, n_nodes=3, tree_off=p, n_trees=1, value=p, n_classes=3, node_weight=p, impurity=None, f=4,
                 per_tree=p, importances=p, n_used=p)
        a.update(kw)
        return tuple(a.values())

    calls = {
        "hypel_forest_oob_rows": [
            oob(x=None), oob(weight=None), oob(out=None), oob(proba=None), oob(votes=None), oob(tree_off=None),
            oob(nodes=None), oob(leaf_value=None), oob(n=0), oob(f=0), oob(ld=3), oob(ldw=7), oob(n_trees=0),
            oob(n_classes=0), oob(n_classes=33), oob(n_leaves=4), oob(nodes=p + 4), oob(nodes=p + 8)],
        "hypel_forest_permuted_hits": [
            hits(x=None), hits(y=None), hits(partner=None), hits(hits=None), hits(nodes=None), hits(n=0), hits(ld=3),
            hits(n_repeats=0), hits(group_mod=0), hits(group_mod=-4), hits(g0=-1), hits(n_groups=0), hits(g0=1),
            hits(n_groups=5), hits(n_classes=33), hits(nodes=p + 8),
            hits(group_mod=1 << 30, n_groups=1 << 30, n_repeats=4), hits(n=1 << 40, ld=4, n_groups=1, n_repeats=1)],
        "hypel_forest_importances_f64": [
            imp(nodes=None), imp(tree_off=None), imp(node_weight=None), imp(per_tree=None), imp(importances=None),
            imp(n_used=None), imp(value=None), imp(n_classes=0), imp(n_classes=33), imp(f=0), imp(n_trees=0),
            imp(n_nodes=0), imp(nodes=p + 4), imp(nodes=p + 8)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
    assert lib.hypel_forest_permuted_hits(*hits(group_mod=1 << 30, n_groups=1 << 30, n_repeats=4), None) == -1
    assert "2^31" in lib.hypel_last_error().decode()
