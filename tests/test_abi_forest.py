"""CPU: the random-forest entry points are declared in include/hypel.h, exported by the library (their binding:
tests/test_abi.py, which checks every prototype of the header), and refuse null pointers, zero or negative sizes,
n_classes above the LDS cap, max_features > F and node records off their 16-byte alignment with a message before
anything is launched.  The ABI version is still 8: new symbols only."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_forest_bin_edges_f32", "hypel_forest_bin_u8", "hypel_forest_split_hist", "hypel_forest_split_apply",
       "hypel_forest_predict_rows", "hypel_forest_predict_scene")


def test_version_8_new_symbols_and_constants(lib):  # noqa: F811
    from hypelcnn_amd import backend
    src = open(HEADER).read()
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", src).group(1))
    assert header == backend.ABI_VERSION == lib.hypel_version() == 8
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name)
    define = lambda k: int(re.search(r"#define\s+HYPEL_FOREST_" + k + r"\s+(\d+)", src).group(1))  # noqa: E731
    assert backend.FOREST_NODE_DTYPE.itemsize == 16 and backend.FOREST_NODE_DTYPE.fields["left"][1] == 8
    assert (define("EDGE_ROWS"), define("MAX_EDGES"), define("MAX_CLASSES"), define("MAX_DEPTH")) == \
        (backend.FOREST_EDGE_ROWS, backend.FOREST_MAX_EDGES, backend.FOREST_MAX_CLASSES, backend.FOREST_MAX_DEPTH) == \
        (16384, 255, 32, 64)


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * (4096 + 16))()
    p = (ctypes.addressof(buf) + 15) // 16 * 16  # never dereferenced: every call below fails its argument check first
    q = p + 2048
    too_many = 33

    def hist(**kw):
        a = dict(bins=p, ldn=8, y=p, weight=p, n=8, n_classes=3, order=p, active=p, n_active=1, cand=p, max_features=2,
                 f=4, score=p, best_bin=p, valid=p)
        a.update(kw)
        return tuple(a.values())

    def apply(**kw):
        a = dict(bins=p, ldn=8, y=p, weight=p, n=8, n_classes=3, order_in=p, order_out=q, active=p, n_active=1, cand=p,
                 max_features=2, f=4, score=p, best_bin=p, valid=p, edges=p, level=0, max_depth=64, node_base=1,
                 node_capacity=15, feature=p, thr_bin=p, threshold=p, left=p, right=p, node_tree=p, node_count=p,
                 node_weight=p, value=p, split_ws=p, next_active=p, counter=p)
        a.update(kw)
        return tuple(a.values())

    def rows(**kw):
        a = dict(x=p, ld=4, n=8, f=4, tree_off=p, n_trees=1, nodes=p, n_nodes=3, leaf_value=p, n_leaves=2, n_classes=3,
                 class_labels=None, points=None, out=p, raster_w=0, proba=None)
        a.update(kw)
        return tuple(a.values())

    def scene(**kw):
        a = dict(casi=p, lidar=p, hp=9, wp=9, cc=3, cl=1, points=p, n=8, p=5, tree_off=p, n_trees=1, scene_nodes=p,
                 n_nodes=3, leaf_value=p, n_leaves=2, n_classes=3, class_labels=None, out=p, raster_w=5)
        a.update(kw)
        return tuple(a.values())

    calls = {
        "hypel_forest_bin_edges_f32": [
            (None, 4, 8, 4, p, 256, p, p), (p, 4, 8, 4, None, 256, p, p), (p, 4, 8, 4, p, 256, None, p),
            (p, 4, 8, 4, p, 256, p, None), (p, 4, 0, 4, p, 256, p, p), (p, 4, -8, 4, p, 256, p, p),
            (p, 4, 8, 0, p, 256, p, p), (p, 3, 8, 4, p, 256, p, p), (p, 4, 8, 4, p, 1, p, p), (p, 4, 8, 4, p, 257, p, p)],
        "hypel_forest_bin_u8": [
            (None, 4, 8, 4, p, p, p, 8), (p, 4, 8, 4, None, p, p, 8), (p, 4, 8, 4, p, None, p, 8),
            (p, 4, 8, 4, p, p, None, 8), (p, 4, 0, 4, p, p, p, 8), (p, 4, 8, -4, p, p, p, 8), (p, 4, 8, 4, p, p, p, 7),
            (p, 3, 8, 4, p, p, p, 8)],
        "hypel_forest_split_hist": [
            hist(bins=None), hist(y=None), hist(weight=None), hist(order=None), hist(active=None), hist(cand=None),
            hist(score=None), hist(best_bin=None), hist(valid=None), hist(n=0), hist(n=-8), hist(ldn=7),
            hist(n_active=0), hist(n_active=-1), hist(n_classes=0), hist(n_classes=too_many), hist(max_features=0),
            hist(max_features=5), hist(f=0)],
        "hypel_forest_split_apply": [
            apply(bins=None), apply(y=None), apply(weight=None), apply(order_in=None), apply(order_out=None),
            apply(order_out=p), apply(active=None), apply(cand=None), apply(score=None), apply(best_bin=None),
            apply(valid=None), apply(edges=None), apply(feature=None), apply(thr_bin=None), apply(threshold=None),
            apply(left=None), apply(right=None), apply(node_tree=None), apply(node_count=None), apply(node_weight=None),
            apply(value=None), apply(split_ws=None), apply(next_active=None), apply(counter=None), apply(n=0),
            apply(ldn=7), apply(n_active=0), apply(n_classes=0), apply(n_classes=too_many), apply(max_features=0),
            apply(max_features=5), apply(level=-1), apply(max_depth=-1), apply(max_depth=65), apply(node_base=-1),
            apply(node_base=16)],
        "hypel_forest_predict_rows": [
            rows(x=None), rows(out=None), rows(tree_off=None), rows(nodes=None), rows(leaf_value=None), rows(n=0),
            rows(n=-1), rows(f=0), rows(ld=3),
            rows(n_trees=0), rows(n_nodes=0), rows(n_leaves=0), rows(n_leaves=4), rows(n_classes=0),
            rows(n_classes=too_many), rows(points=p, raster_w=0), rows(nodes=p + 4), rows(nodes=p + 8)],
        "hypel_forest_predict_scene": [
            scene(casi=None), scene(lidar=None), scene(points=None), scene(out=None), scene(tree_off=None),
            scene(scene_nodes=None), scene(leaf_value=None), scene(n=0), scene(p=0), scene(hp=4), scene(wp=4),
            scene(cc=0), scene(cl=-1),
            scene(raster_w=0), scene(n_trees=0), scene(n_leaves=0), scene(n_classes=0), scene(n_classes=too_many),
            scene(hp=-9), scene(scene_nodes=p + 4), scene(scene_nodes=p + 8)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
