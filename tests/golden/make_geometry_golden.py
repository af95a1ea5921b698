#!/usr/bin/env python3
"""Generates tests/golden/geometry_golden.npz by running the REFERENCE ITSELF (oracle/_ref/libmpl_ref.so: the
reference's own headers compiled where they lie, see oracle/ref_shim.cpp and make_golden.py) on the anisotropic worlds
of tests/test_gpu_map_geometry.py:

    python tests/golden/make_geometry_golden.py

Per world: the dense status (uint8) and iteration counts (uint8: a primitive has at most 61 + 1 samples here, checked)
and SHA-256 digests of the hash and cost bytes -- 136 worlds stay below the size of get_succ_golden.npz that way --
plus digests of the world's own nodes and cells, so that a changed builder shows as such and not as a wrong result.
The worlds come from the test module's builder; the fixture pins what the reference answered for them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import oracle as O  # noqa: E402
import motion_primitive_library_amd as m  # noqa: E402
from helpers import oracle_env  # noqa: E402
from test_gpu_map_geometry import WORLDS, digest, make_world, world_name  # noqa: E402


def main():
    O.build(ref=True)
    out = {}
    names = []
    for dims, cfg in WORLDS:
        wl = make_world(m, dims, cfg)
        r = O.expand(oracle_env(wl), wl.nodes, threads=1, ref=True)
        name = world_name(dims, cfg)
        names.append(name)
        assert 0 <= r["iters"].min() and r["iters"].max() < 256
        out[name + "/status"] = r["status"]
        out[name + "/iters"] = r["iters"].astype(np.uint8)
        out[name + "/hash_sha256"] = digest(r["hash"])
        out[name + "/cost_sha256"] = digest(r["cost"])
        out[name + "/nodes_sha256"] = digest(wl.nodes)
        out[name + "/grid_sha256"] = digest(np.ascontiguousarray(wl.grid, dtype=np.int8))
    out["names"] = np.array(names)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "geometry_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d worlds, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
