"""Records tests/golden/png_metrics.npz with Pillow: a few uint8 RGB images, Pillow's `convert('L')` of each, and the same after a PNG
round trip through BytesIO (what upstream Vid-ODE's evaluate.py reads back from the files save_image wrote).  The fixture pins the
integer luma restatement of tests/_png_metrics_ref.py without needing Pillow where the tests run.

    python tests/golden/make_golden_png_metrics.py
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def images():
    rng = np.random.default_rng(20251019)
    out = {"random64": rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)}
    y, x = np.mgrid[0:64, 0:64]
    out["ramps64"] = np.stack([4 * x, 4 * y, (x * y) % 256], axis=-1).astype(np.uint8)              # every value of R and G, a sawtooth in B
    grey = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    out["grey64"] = np.stack([grey] * 3, axis=-1)                                                     # R = G = B: L must equal R
    big = rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:128, 0:128]
    big[32:96, 32:96] = np.stack([2 * xx[32:96, 32:96], 255 - 2 * yy[32:96, 32:96], (xx + yy)[32:96, 32:96]], axis=-1).astype(np.uint8)
    out["mixed128"] = big
    return out


def main():
    blob = {}
    for name, rgb in images().items():
        direct = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
        buf = io.BytesIO()
        Image.fromarray(rgb, "RGB").save(buf, format="PNG")
        buf.seek(0)
        back = Image.open(buf)
        assert np.array_equal(np.asarray(back.convert("RGB")), rgb), "a PNG round trip is lossless"
        blob[f"{name}.rgb"], blob[f"{name}.luma"], blob[f"{name}.luma_png"] = rgb, direct, np.asarray(back.convert("L"))
    np.savez_compressed(os.path.join(HERE, "png_metrics.npz"), **blob)
    print({k: v.shape for k, v in blob.items()})


if __name__ == "__main__":
    main()
