#!/usr/bin/env python3
"""Generate tests/golden/ingest_data.npz: the reference's CPU float32 output of a data-dependent normalisation.

TEST INFRASTRUCTURE, build-container only, like make_golden.py (whose stand-in modules and reference path it reuses):
the reference's own ``normalize_tensor`` (clair_torch/common/general_functions.py:359-388) with ``max_val`` and / or
``min_val`` None -- the bound is then the tensor's own extremum -- run on float32 CPU tensors.  Only the outputs are
committed; the inputs are rebuilt from the recorded seed by ``stack`` below, which the host test imports.

Run:  python tests/golden/make_golden_ingest_data.py            (writes next to this file)
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (seed, dtype, shape, top code / scale, max_val, min_val, target range)
CASES = {
    "u16_default": (101, "uint16", (2, 3, 5, 7), 5000, None, None, (0.0, 1.0)),
    "u8_none_0": (102, "uint8", (1, 3, 4, 9), 200, None, 0, (0.0, 1.0)),
    "u16_4095_none_pm1": (103, "uint16", (3, 1, 6, 5), 4500, 4095, None, (-1.0, 1.0)),
    "f32_default_range": (104, "float32", (2, 2, 3, 5), 5000.0, None, None, (0.25, 0.75)),
    "f32_none_min": (105, "float32", (1, 3, 7, 3), 3.0, None, -1.5, (0.0, 1.0)),
}


def stack(name):
    """The input of case ``name`` as a numpy array of its own dtype (integer codes 16..top, floats in [-top/25, top))."""
    seed, dtype, shape, top = CASES[name][:4]
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        return (rng.random(shape, dtype=np.float32) * np.float32(top * 1.04) - np.float32(top * 0.04)).astype(np.float32)
    return rng.integers(16, top + 1, size=shape).astype(dtype)


def main():
    sys.path.insert(0, HERE)
    import make_golden  # noqa: F401  (installs the stand-ins and puts the reference on sys.path)
    import torch
    from clair_torch.common.general_functions import normalize_tensor
    out = {}
    for name, (_, _, _, _, mx, mn, rng) in CASES.items():
        x = torch.from_numpy(stack(name).astype(np.float32))
        out[name] = normalize_tensor(x, mx, mn, rng).numpy()
        assert out[name].dtype == np.float32
    path = os.path.join(HERE, "ingest_data.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
