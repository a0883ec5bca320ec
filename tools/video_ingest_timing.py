"""Time ct_video_stats_ingest_batch against the two launches it replaces -- ct_ingest_transform into a float32 stack, then
the float32 ct_video_stats_batch on that stack (what compute_video_mean_and_std(fused_ingest=False) runs) -- on the same
resident data, on the same device, in the same process.

    python tools/video_ingest_timing.py [--blocks 15] [--inner 250] [--warmup 3] [--out FILE.json]

Batches of 32 frames 3 x 1080 x 1920, uint16 and uint8, planar (B,C,H,W) and BGR-interleaved (B,H,W,3) behind CvToTorch; the
list is ``[CastTo(float32), Normalize(1023, 64), ClampAlongDims(1, three pairs)]`` (``Normalize(255, 16)`` for uint8, whose
codes end at 255), LINEAR, 256 points, three different rows.  The state holds 32 frames already (``frames_before = 32``), so
every launch reads and writes it, as all but the first batch of a video do.

Method: device events around ``--inner`` launches in a row on one stream (250: a block is 50 - 100 ms, a candidate gets more
than a second per case), the two candidates alternating block by block so that both see the same clocks and neighbours;
``--warmup`` blocks of each are dropped, the median / min / max per batch is taken over the other ``--blocks``.
``pair_spread`` is (max - min) / median of the pair's blocks: the fused launch counts as
faster only where ``pair_over_fused - 1`` exceeds it.  The states of the two candidates are compared after the first
launch (``differing`` must be 0).  The byte floor is B * sizeof(code) + 16 B of state per element, every byte once, over
the 8 TB/s HBM peak of the MI355X.  One JSON line on stdout (and in ``--out``)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402
from clair_torch_amd.common.transforms import CastTo, ClampAlongDims, CvToTorch, Normalize, plan_staging  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
B, C, H, W = 32, 3, 1080, 1920
PAIRS = [(0.0, 1.0), (0.02, 0.9), (0.05, 0.8)]


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
    return a.elapsed_time(b) / inner  # ms per batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--inner", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    result = {"device": torch.cuda.get_device_name(dev), "batch": [B, C, H, W], "blocks": args.blocks, "inner": args.inner, "cases": []}
    for dtype in (torch.uint16, torch.uint8):
        top, black = (1023, 64) if dtype == torch.uint16 else (255, 16)
        for layout in ("nchw", "nhwc_bgr"):
            x = _draw((B, C, H, W) if layout == "nchw" else (B, H, W, C), dtype, dev)
            lead = [CvToTorch()] if layout != "nchw" else []
            plan = plan_staging(x, lead + [CastTo("float32"), Normalize(top, black), ClampAlongDims(1, PAIRS)])
            assert plan.route == "ingest" and plan.source_layout == layout and len(plan.stages) == 2
            staged = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
            start = [torch.rand((C, H, W), device=dev), torch.rand((C, H, W), device=dev)]
            state_f = [t.clone() for t in start]
            state_p = [t.clone() for t in start]

            def fused():
                ops.video_stats_ingest_batch(x, plan.stages, state_f[0], state_f[1], B, lut=lut, interp="linear", layout=layout)

            def pair():
                ops.ingest_transform(x, plan.stages, layout=layout, out=staged)
                ops.video_stats_batch(staged, state_p[0], state_p[1], B, lut=lut, interp="linear")

            fused()
            pair()
            differing = int((state_f[0] != state_p[0]).sum()) + int((state_f[1] != state_p[1]).sum())
            times = {"fused": [], "pair": []}
            for _ in range(args.warmup + args.blocks):  # alternate the candidates: both see the same neighbours and clocks
                times["fused"].append(_block(fused, args.inner))
                times["pair"].append(_block(pair, args.inner))
            floor_bytes = C * H * W * (B * x.element_size() + 16)
            row = {"case": f"{str(dtype).split('.')[-1]} {layout}", "differing": differing, "floor_bytes": floor_bytes,
                   "floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3}
            for name, ts in times.items():
                ts = ts[args.warmup:]
                row.update({f"{name}_ms_median": statistics.median(ts), f"{name}_ms_min": min(ts), f"{name}_ms_max": max(ts)})
            row["pair_spread"] = (row["pair_ms_max"] - row["pair_ms_min"]) / row["pair_ms_median"]
            row["pair_over_fused"] = row["pair_ms_median"] / row["fused_ms_median"]
            row["fused_faster_beyond_spread"] = row["pair_over_fused"] - 1.0 > row["pair_spread"]
            row["fused_share_of_floor"] = row["floor_ms_at_8TBps"] / row["fused_ms_median"]
            result["cases"].append(row)
            del x, staged, state_f, state_p, start
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
