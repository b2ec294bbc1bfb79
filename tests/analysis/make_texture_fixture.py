#!/usr/bin/env python3
"""tests/golden/assets/textures/holz_sampled.png: the theater scene's texture textures/holz.jpg, decoded, with only the pixels its
512 x 512 atlas cell reads kept (the nearest-resample rule of web-ray-tracer_amd/js/sceneFile.js buildAtlas) and every other pixel black.
Lossless and full size, so the test still resamples the image itself: a wrong rule reads a black pixel and the scene's hashes differ.
Authoring only (needs the reference's textures/holz.jpg).

    python tests/analysis/make_texture_fixture.py <reference root>"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CELL = 512                                      # the theater scene's standardTextureSizes


def main():
    src = os.path.join(sys.argv[1], "textures", "holz.jpg")
    im = np.asarray(Image.open(src).convert("RGB"))
    h, w = im.shape[:2]
    sy = np.minimum(h - 1, np.floor((np.arange(CELL) + 0.5) * h / CELL).astype(np.int64))
    sx = np.minimum(w - 1, np.floor((np.arange(CELL) + 0.5) * w / CELL).astype(np.int64))
    out = np.zeros_like(im)
    out[np.ix_(sy, sx)] = im[np.ix_(sy, sx)]
    path = os.path.join(ROOT, "tests", "golden", "assets", "textures", "holz_sampled.png")
    Image.fromarray(out).save(path, "PNG", optimize=True)
    print(path, out.shape, os.path.getsize(path))


if __name__ == "__main__":
    main()
