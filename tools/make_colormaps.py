#!/usr/bin/env python3
"""Writes mindtheedge_amd/utils/colormaps.json (text: one "[r, g, b]" row per line, floats in their shortest exact form, so that the file
reads back to the same float64 bits): the 256 x 3 float64 RGB tables of matplotlib's ``plasma`` (a listed map) and ``Spectral``
(a segmented map, sampled at its default N = 256), the two maps the reference's inference side colours depth with
(utils/depth.py::viz_inv_depth, infer_edges.py:355-366).  The package and its GPU tests read the file and never import matplotlib;
tests/test_viz_ref_cpu.py compares the file with the installed matplotlib when there is one.

    python tools/make_colormaps.py          # generated with matplotlib 3.10.8
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mindtheedge_amd", "utils", "colormaps.json")
NAMES = ("plasma", "Spectral")


def tables():
    import matplotlib
    out = {}
    for name in NAMES:
        cm = matplotlib.colormaps[name]
        t = np.asarray(cm(np.arange(256)), dtype=np.float64)[:, :3]          # integer input: the look-up table rows themselves
        assert cm.N == 256 and t.shape == (256, 3)
        out[name] = np.ascontiguousarray(t)
    return out


def dumps(version, named):
    import json
    parts = ['  "matplotlib_version": %s' % json.dumps(version)]
    for name, t in named.items():
        rows = ",\n".join("    " + json.dumps([float(v) for v in row]) for row in t)
        parts.append('  %s: [\n%s\n  ]' % (json.dumps(name), rows))
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    import json
    import matplotlib
    text = dumps(matplotlib.__version__, tables())
    back = json.loads(text)
    assert all(np.array_equal(np.array(back[k], dtype=np.float64), v) for k, v in tables().items())      # exact round trip
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT)
