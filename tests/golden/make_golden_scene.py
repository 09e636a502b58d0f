#!/usr/bin/env python3
"""Generate tests/golden/scene_tiles.npz from the REFERENCE's own tiler.

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_scene.py

``splitbase.SplitSingle`` (DOTA_devkit/SplitOnlyImage_multi_process.py:51-85) is imported in place with stub modules
for the absent third-party cv2 / shapely; ``cv2.imread`` returns a zero image of the wanted size and
``saveimagepatches`` is replaced by a recorder, so the fixture holds exactly the (left, up) origins and chip names
the script would have written chips for.  DATA only: extents, gaps, origins, names.
"""
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("S2A_REFERENCE", "/root/reference")

EXTENTS = (600, 1024, 1025, 1849, 2500, 4096)
NON_SQUARE = ((600, 900), (1025, 1849), (2500, 1800))       # (height, width)
GAPS = (200, 100)
RATES = (1, 0.5, 1.5)                                        # as splitdata(1) / (0.5) / (1.5) pass them: names only


def import_splitbase():
    sys.dont_write_bytecode = True
    cv2 = types.ModuleType("cv2")
    cv2.INTER_CUBIC = 2
    sh = types.ModuleType("shapely")
    sh.geometry = types.ModuleType("shapely.geometry")
    sys.modules.setdefault("cv2", cv2)
    sys.modules.setdefault("shapely", sh)
    sys.modules.setdefault("shapely.geometry", sh.geometry)
    sys.path.insert(0, os.path.join(REF, "DOTA_devkit"))
    import SplitOnlyImage_multi_process as mod
    return mod


def record(mod, height, width, gap, rate=1, subsize=1024, name="P0001"):
    sb = mod.splitbase.__new__(mod.splitbase)               # (no worker pool, no output directory)
    sb.srcpath = sb.outpath = sb.dstpath = ""
    sb.gap, sb.subsize, sb.slide, sb.ext, sb.padding = gap, subsize, subsize - gap, ".png", True
    seen = []
    sb.saveimagepatches = lambda img, subimgname, left, up, ext=".png": seen.append((int(left), int(up), subimgname))
    mod.cv2.imread = lambda path: np.zeros((height, width, 3), np.uint8)
    # the resize of rate != 1 is the caller's business (cv2 is absent): the scene handed over IS the resized one
    mod.cv2.resize = lambda img, dsize, fx, fy, interpolation: img
    sb.SplitSingle(name, rate, ".png")
    return np.asarray([s[:2] for s in seen], np.int32).reshape(-1, 2), [s[2] for s in seen]


def main():
    assert os.path.isdir(REF), "run in the build container (needs the reference checkout)"
    mod = import_splitbase()
    cases = [(e, e) for e in EXTENTS] + list(NON_SQUARE)
    # every extent on either axis against a different one on the other (both loop orders show)
    cases += [(EXTENTS[i], EXTENTS[(i + 2) % len(EXTENTS)]) for i in range(len(EXTENTS))]
    out = {}
    meta = []
    for gap in GAPS:
        for k, (h, w) in enumerate(cases):
            rate = RATES[k % len(RATES)]
            origins, names = record(mod, h, w, gap, rate)
            key = "g%d_h%d_w%d" % (gap, h, w)
            out[key + "_origins"] = origins
            out[key + "_names"] = np.asarray(names)
            meta.append((h, w, gap, 1024, str(rate)))
            print(key, "rate", rate, len(names), "tiles")
    out["cases"] = np.asarray(meta)                          # rows of strings: height, width, gap, subsize, str(rate)
    out["image_name"] = np.asarray("P0001")
    np.savez_compressed(os.path.join(OUT, "scene_tiles.npz"), **out)


if __name__ == "__main__":
    main()
