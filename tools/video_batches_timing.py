"""Time a stream of small video batches through ct_video_stats_batches / ct_video_stats_ingest_batches (several batches per
launch, the running state in registers in between) against one launch per batch through the single-batch entry points --
what compute_video_mean_and_std does by default -- on the same resident data, on the same device, in the same process.

    python tools/video_batches_timing.py [--blocks 9] [--inner 8] [--warmup 2] [--out FILE.json]

64 batches of 4 frames 3 x 1080 x 1920 (the reference's ``batch_size: 4``), uint16 and uint8, planar (B,C,H,W) and
BGR-interleaved (B,H,W,3) behind CvToTorch; "ingest": the list ``[CastTo(float32), Normalize(1023, 64)]`` (``Normalize(255,
16)`` for uint8) on route "ingest", evaluated inside the kernel; "code": the pair ``[CastTo(float32), Normalize(max, 0)]`` on
route "code".  LINEAR, 256 points, three different rows.  The state holds 4 frames already, so every launch reads it.

Three configurations: ``per_batch`` (64 launches: the baseline), ``groups_of_4`` (16 launches), ``groups_of_16`` (4 launches).

Method: device events around ``--inner`` whole streams in a row on one stream, the three configurations alternating block by
block so that all see the same clocks and neighbours; ``--warmup`` blocks of each are dropped, the median / min / max per
stream is taken over the other ``--blocks``.  The time is that of the whole stream as the host issues it, front-end checks
and launch cost included.  ``spread`` is (max - min) / median of the baseline's blocks: a grouped configuration counts as
faster only where ``1 - ratio`` exceeds it.  The states are compared after the first stream (``differing`` must be 0).  The
byte model per element: 64 * 4 * sizeof(code) of samples plus 16 B of state per launch; GB/s is that over the median."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402
from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize, plan_staging  # noqa: E402

N_BATCHES, B, C, H, W = 64, 4, 3, 1080, 1920
GROUPS = {"per_batch": 1, "groups_of_4": 4, "groups_of_16": 16}


def _draw(shape, dtype, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    if dtype == torch.uint16:  # torch draws no uint16: codes 0 .. 1099 through the int16 view
        return torch.randint(0, 1100, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    return torch.randint(0, 256, shape, dtype=dtype, device=dev, generator=gen)


def _block(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner  # ms per stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    result = {"device": torch.cuda.get_device_name(dev), "stream": [N_BATCHES, B, C, H, W], "blocks": args.blocks, "inner": args.inner,
              "cases": []}
    for dtype in (torch.uint16, torch.uint8):
        top, black = (1023, 64) if dtype == torch.uint16 else (255, 16)
        for layout in ("nchw", "nhwc_bgr"):
            frames = _draw((N_BATCHES * B, C, H, W) if layout == "nchw" else (N_BATCHES * B, H, W, C), dtype, dev)
            batches = [frames[k * B:(k + 1) * B] for k in range(N_BATCHES)]
            lead = [CvToTorch()] if layout != "nchw" else []
            for route in ("ingest", "code"):
                plan = plan_staging(batches[0], lead + [CastTo("float32"), Normalize(top, black if route == "ingest" else 0)])
                assert plan.route == route and (plan.source_layout if route == "ingest" else plan.layout) == layout
                start = [torch.rand((C, H, W), device=dev), torch.rand((C, H, W), device=dev)]
                states = {name: [t.clone() for t in start] for name in GROUPS}
                kw = dict(lut=lut, interp="linear", layout=layout)

                def stream(name):
                    mean, m2 = states[name]
                    g = GROUPS[name]
                    for k in range(0, N_BATCHES, g):
                        before = B + k * B
                        if route == "ingest":
                            if g == 1:
                                ops.video_stats_ingest_batch(batches[k], plan.stages, mean, m2, before, **kw)
                            else:
                                ops.video_stats_ingest_batches(batches[k:k + g], plan.stages, mean, m2, before, require_one_launch=True, **kw)
                        elif g == 1:
                            ops.video_stats_batch(batches[k], mean, m2, before, max_code=plan.max_code, **kw)
                        else:
                            ops.video_stats_batches(batches[k:k + g], mean, m2, before, max_code=plan.max_code, require_one_launch=True, **kw)

                for name in GROUPS:
                    stream(name)
                differing = sum(int((states[name][i] != states["per_batch"][i]).sum()) for name in GROUPS for i in (0, 1))
                times = {name: [] for name in GROUPS}
                for _ in range(args.warmup + args.blocks):  # alternate the configurations: all see the same neighbours and clocks
                    for name in GROUPS:
                        times[name].append(_block(lambda: stream(name), args.inner))
                row = {"case": f"{str(dtype).split('.')[-1]} {layout} {route}", "differing": differing}
                for name, g in GROUPS.items():
                    ts = times[name][args.warmup:]
                    model_bytes = C * H * W * (N_BATCHES * B * frames.element_size() + 16 * (N_BATCHES // g))
                    med = statistics.median(ts)
                    row[name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "model_bytes": model_bytes,
                                 "model_GBps": model_bytes / med / 1e6}
                base = row["per_batch"]
                row["spread"] = (base["ms_max"] - base["ms_min"]) / base["ms_median"]
                for name in ("groups_of_4", "groups_of_16"):
                    row[name]["ratio"] = row[name]["ms_median"] / base["ms_median"]
                    row[name]["model_ratio"] = row[name]["model_bytes"] / base["model_bytes"]
                    row[name]["faster_beyond_spread"] = 1.0 - row[name]["ratio"] > row["spread"]
                result["cases"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del states, start
            del frames, batches
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
