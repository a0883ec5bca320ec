"""Time one train_icrf step (staging + linearity forward + backward) on raw uint16 codes behind a black-level chain, at the
shape of BASELINE configuration C3, planar and as raw BGR frames; prints one JSON line per case and run.

    python tools/pairs_ingest_timing.py [--fused 0|1] [--exposures 64] [--size 2048] [--steps 10] [--warmup 3] [--repeats 3]

The step is the body of train_icrf's batch loop with the batch already resident on the device (the host-to-device copy is
the same on every route): stage the batch, linearity_loss, backward.  hipEvent pairs around `steps` warm steps; peak device
memory from torch.cuda.max_memory_allocated.  The script also runs on a checkout from before the fused route existed (no
``stage_pair_images``): it then times what that checkout does, which is the comparand -- never time the two routes of one
checkout against each other to judge the fused one.  profiles/pairs_ingest.md holds the figures."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", type=int, default=1)
    ap.add_argument("--exposures", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from clair_torch_amd import ops
    from clair_torch_amd.common import transforms as T
    from clair_torch_amd.common.general_functions import get_valid_exposure_pairs
    from clair_torch_amd.datasets import synthetic_exposure_stack
    from clair_torch_amd.inference._staging import stage_images
    from clair_torch_amd.training import linearity
    dev = torch.device("cuda:0")
    has_fused = hasattr(linearity, "stage_pair_images")
    n = args.exposures
    codes, exposures = synthetic_exposure_stack(n, 3, args.size, args.size, bits=16, stops_per_step=0.125, seed=1237, device=dev)
    t = torch.tensor(exposures, dtype=torch.float64)
    pairs = ops.PairList(*get_valid_exposure_pairs(t, 0.25), n, dev)
    lut = (torch.linspace(0, 1, 256, device=dev) ** 2.5).repeat(3, 1).contiguous().requires_grad_(True)
    chain = [T.CastTo("float32"), T.Normalize(65535, 64)]
    cases = {"planar": (codes, chain)}
    bgr = codes.to(torch.int32).flip(1).permute(0, 2, 3, 1).contiguous().to(torch.uint16)
    cases["nhwc_bgr"] = (bgr, [T.CvToTorch()] + chain)

    def step(batch, transforms):
        if has_fused:
            images, max_code, layout, _ = linearity.stage_pair_images(batch, dev, transforms, False, bool(args.fused))
        else:
            images, max_code, layout = stage_images(batch, dev, transforms, planar=False)
        lin, _ = linearity.linearity_loss(lut, images, pairs, interp="linear", lower=1 / 255, upper=254 / 255, use_relative=True,
                                          use_unc_weight=False, max_code=max_code, group=False, layout=layout)
        lut.grad = None
        lin.sum().backward()
        return lin

    for name, (batch, transforms) in cases.items():
        for _ in range(args.warmup):
            lin = step(batch, transforms)
        torch.cuda.synchronize()
        for run in range(args.repeats):
            torch.cuda.reset_peak_memory_stats()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.steps):
                lin = step(batch, transforms)
            stop.record()
            torch.cuda.synchronize()
            print(json.dumps({"case": name, "route": ("fused" if args.fused else "two launches") if has_fused else "before the fused route",
                              "run": run, "ms_per_step": round(start.elapsed_time(stop) / args.steps, 3),
                              "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
                              "pairs": pairs.n_pairs, "loss": [round(float(v), 9) for v in lin.detach().cpu()]}), flush=True)


if __name__ == "__main__":
    main()
