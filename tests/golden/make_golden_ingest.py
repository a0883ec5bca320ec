#!/usr/bin/env python3
"""Generate tests/golden/ingest.npz: the reference's CPU float32 output of the transforms the fused ingest evaluates.

TEST INFRASTRUCTURE, build-container only, like make_golden.py (whose stand-in modules and reference path it reuses):
the reference's own ``normalize_tensor`` / ``clamp_along_dims`` (clair_torch/common/general_functions.py:359-436) run
on float32 CPU tensors; only the recorded outputs are committed.  Inputs are not stored: they are every code in order
and a ramp rebuilt from the recorded parameters.

Run:  python tests/golden/make_golden_ingest.py            (writes next to this file)
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stand-ins and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from clair_torch.common.general_functions import clamp_along_dims, normalize_tensor  # noqa: E402

U8_PARAMS = (255, 16, (0.0, 1.0))
U16_PARAMS = {"u16_65535_256": (65535, 256, (0.0, 1.0)), "u16_4095_64_pm1": (4095, 64, (-1.0, 1.0))}
CLAMP_PAIRS = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]
RAMP = (-0.5, 1.5, 4096)  # torch.linspace arguments, float32


def main():
    out = {}
    codes8 = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(torch.float32)
    out["u8_255_16"] = normalize_tensor(codes8, *U8_PARAMS).numpy()
    out["u8_255_16_params"] = np.array([U8_PARAMS[0], U8_PARAMS[1], *U8_PARAMS[2]], dtype=np.float64)
    codes16 = torch.arange(65536, dtype=torch.int32).to(torch.float32)
    for name, (mx, mn, rng) in U16_PARAMS.items():
        out[name] = normalize_tensor(codes16, mx, mn, rng).numpy()
        out[name + "_params"] = np.array([mx, mn, *rng], dtype=np.float64)
    ramp = torch.linspace(*RAMP, dtype=torch.float32)
    x = torch.stack([ramp, ramp, ramp]).view(1, 3, 1, -1)
    out["clamp_ramp"] = np.array(RAMP, dtype=np.float64)
    out["clamp_pairs"] = np.array(CLAMP_PAIRS, dtype=np.float64)
    out["clamp_per_channel"] = clamp_along_dims(x, 1, CLAMP_PAIRS).numpy()
    out["clamp_single_pair"] = clamp_along_dims(x, 0, CLAMP_PAIRS[1]).numpy()
    for v in out.values():
        assert v.dtype in (np.float32, np.float64)
    path = os.path.join(HERE, "ingest.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
