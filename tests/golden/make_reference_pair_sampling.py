#!/usr/bin/env python3
"""Pin the shadow / lit pairing by executing the reference's own samplers (build container only; needs
/root/reference).

`gan/gan_sampling_methods.py` runs UNCHANGED -- NeighborhoodBasedSampler, RandomBasedSampler and TargetBasedSampler --
on the seeded scenes of tests/pair_cases.py through stub data sets and loaders.  The reference writes `numpy.int`, which
NumPy 2 no longer has: it is set to `int` before the import.

Written to tests/golden/reference_pair_sampling.json / .npz: per scene the prepared casi / lidar arrays, the shadow map
and the target list; per case the two pair arrays the sampler returned.  Only data is written."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from tests import pair_cases as C  # noqa: E402


def main():
    if not os.path.isdir(REF):
        raise RuntimeError("the reference is only present in the build container")
    np.int = int
    sys.path.insert(0, REF)
    ref = importlib.import_module("gan.gan_sampling_methods")
    assert os.path.abspath(ref.__file__).startswith(REF)
    arrays, meta = {}, {"scenes": {}, "cases": {}}
    scenes = {}
    for name in C.SCENES:
        s = scenes[name] = C.build_scene(name)
        for key in ("casi", "lidar", "map", "targets"):
            if s[key] is not None:
                arrays[f"scene/{name}/{key}"] = s[key]
        meta["scenes"][name] = {"neighborhood": s["neighborhood"], "classes": s["classes"], "h": s["h"], "w": s["w"],
                                "has_lidar": s["lidar"] is not None}
    for case, (scene, cls, kwargs) in C.CASES.items():
        s = scenes[scene]
        data_set, loader = C.stubs(s)
        normal, shadow = getattr(ref, cls)(**kwargs).get_sample_pairs(data_set, loader, s["map"].copy())
        arrays[f"case/{case}/normal"] = np.asarray(normal)
        arrays[f"case/{case}/shadow"] = np.asarray(shadow)
        meta["cases"][case] = {"scene": scene, "sampler": cls, "args": kwargs, "normal": list(np.shape(normal)),
                               "shadow": list(np.shape(shadow))}
    with open(os.path.join(HERE, "reference_pair_sampling.json"), "w") as f:
        json.dump(meta, f, sort_keys=True, indent=0, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "reference_pair_sampling.npz"), **arrays)
    print("wrote reference_pair_sampling.json / .npz:", len(arrays), "arrays")
    for case, m in meta["cases"].items():
        print(" ", case, m["normal"], m["shadow"])


if __name__ == "__main__":
    main()
