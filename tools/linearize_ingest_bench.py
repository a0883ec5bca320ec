"""Time ct_linearize_ingest against the two launches it replaces -- ct_ingest_transform into a float32 stack, then
ct_linearize_std on that stack -- on the same device in the same process, and linearize_dataset_generator's pipelined
route against its frame-by-frame route for the same list (profiles/linearize_ingest.md).

    python tools/linearize_ingest_bench.py [--launches 30] [--warmup 5] [--frames 64] [--skip-end-to-end] [--out FILE.json]

The list is ``[CastTo(float32), Normalize(4095, 64), ClampAlongDims(1, 3 pairs)]`` (``Normalize(255, 16)`` for uint8), behind
``CvToTorch`` for the raw (F,H,W,3) BGR frames; LINEAR, 256 points, MULTIPLIER 0.05.  Kernel only: device-event time of
every run, the two candidates alternating, median after warm-up; the byte floor is ``sizeof(T) + 8`` bytes per sample,
every byte once, over the 8 TB/s HBM peak of the MI355X.  The outputs are also compared (``differing`` must be 0).  End
to end: frames per second of the generator over pinned 1080p uint16 frames, host clock around the whole run (it ends with
the last device-to-host copy), the two routes alternating; the frame-by-frame figure is taken by patching
``pipeline_route`` to decline.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402
from clair_torch_amd.common.enums import InterpMode, MissingStdMode  # noqa: E402
from clair_torch_amd.common.transforms import CastTo, ClampAlongDims, CvToTorch, Normalize, fusable_ingest  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
PAIRS = [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)]
CASES = [((64, 3, 1080, 1920), torch.uint16, 4500), ((64, 3, 1080, 1920), torch.uint8, 255), ((32, 3, 4096, 4096), torch.uint16, 4500)]


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _draw(shape, dtype, top, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    if dtype == torch.uint16:  # torch draws no uint16: the codes fit the positive half of int16
        return torch.randint(0, top + 1, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    return torch.randint(0, top + 1, shape, dtype=dtype, device=dev, generator=gen)


def _chain(dtype):
    return [CastTo("float32"), Normalize(4095 if dtype == torch.uint16 else 255, 64 if dtype == torch.uint16 else 16),
            ClampAlongDims(1, PAIRS)]


def kernel_only(args, dev, lut):
    results = []
    for (b, c, h, w), dtype, top in CASES:
        layouts = ("nchw", "nhwc_bgr") if h == 1080 else ("nchw",)
        for layout in layouts:
            shape = (b, c, h, w) if layout == "nchw" else (b, h, w, c)
            x = _draw(shape, dtype, top, dev)
            ts = ([CvToTorch()] if layout != "nchw" else []) + _chain(dtype)
            plan = fusable_ingest(x, ts)
            assert plan is not None and plan.layout == layout
            staged = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
            out = (torch.empty_like(staged), torch.empty_like(staged))
            out2 = (torch.empty_like(staged), torch.empty_like(staged))
            kw = dict(std_mode="multiplier", std_value=0.05)

            def fused():
                return ops.linearize_ingest_frames(x, plan.stages, lut, "linear", layout=layout, out=out, **kw)

            def two_launches():
                ops.ingest_transform(x, plan.stages, layout=layout, out=staged)
                return ops.linearize_frames(staged, lut, "linear", out=out2, **kw)

            fused()
            two_launches()
            differing = int((out[0].view(torch.int32) != out2[0].view(torch.int32)).sum()) + \
                int((out[1].view(torch.int32) != out2[1].view(torch.int32)).sum())
            t_f, t_t = [], []
            for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
                t_f.append(_time(fused))
                t_t.append(_time(two_launches))
            t_f, t_t = t_f[args.warmup:], t_t[args.warmup:]
            floor_bytes = x.numel() * (x.element_size() + 8)
            two_bytes = x.numel() * (x.element_size() + 4 + 4 + 8)
            med_f, med_t = statistics.median(t_f), statistics.median(t_t)
            row = {"case": f"{b}x{c}x{h}x{w} {str(dtype).split('.')[-1]} {layout}", "launches": len(t_f),
                   "fused_ms_median": med_f * 1e3, "fused_ms_min": min(t_f) * 1e3, "fused_ms_max": max(t_f) * 1e3,
                   "two_launch_ms_median": med_t * 1e3, "two_launch_ms_min": min(t_t) * 1e3, "two_launch_ms_max": max(t_t) * 1e3,
                   "two_launch_over_fused": med_t / med_f, "floor_bytes": floor_bytes, "two_launch_bytes": two_bytes,
                   "floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3, "fused_floor_TBps": floor_bytes / med_f / 1e12,
                   "fused_share_of_floor": floor_bytes / HBM_PEAK / med_f, "two_launch_TBps": two_bytes / med_t / 1e12,
                   "elements": x.numel(), "differing": differing}
            results.append(row)
            print(json.dumps(row), flush=True)
            del x, staged, out, out2
            torch.cuda.empty_cache()
    return results


def end_to_end(args, dev, lut):
    """frames / s of linearize_dataset_generator for the list, pipelined against frame by frame, on pinned 1080p frames."""
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    n = args.frames
    codes = _draw((n, 3, 1080, 1920), torch.uint16, 4500, dev).cpu().pin_memory()
    ds = StackDataset(codes, [float(k + 1) for k in range(n)], missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                      materialize_std=False)
    model = ICRFModelDirect(icrf=lut.cpu(), interpolation_mode=InterpMode.LINEAR).to(dev)
    ts = _chain(torch.uint16)
    decide = linearization.pipeline_route

    def run(route):
        linearization.pipeline_route = decide if route == "pipelined" else (lambda probe, plan, has_dark: "frame_by_frame")
        try:
            loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count, check = 0, 0.0
            for lin, sd, _ in linearize_dataset_generator(loader, "cuda", model, gpu_transforms=ts):
                count += 1
                check += float(lin[0, 0, 0]) + float(sd[0, 0, 0])
            torch.cuda.synchronize()
            return count / (time.perf_counter() - t0), check
        finally:
            linearization.pipeline_route = decide

    rates = {"pipelined": [], "frame_by_frame": []}
    checks = {}
    for rep in range(args.repeats + 1):  # the first round warms both routes up
        for route in rates:
            fps, check = run(route)
            checks[route] = check
            if rep:
                rates[route].append(fps)
    row = {"case": f"end to end, {n} pinned frames 3x1080x1920 uint16, [CastTo, Normalize(4095, 64), ClampAlongDims]",
           "repeats": args.repeats,
           "pipelined_fps_median": statistics.median(rates["pipelined"]), "pipelined_fps_min": min(rates["pipelined"]),
           "pipelined_fps_max": max(rates["pipelined"]),
           "frame_by_frame_fps_median": statistics.median(rates["frame_by_frame"]),
           "frame_by_frame_fps_min": min(rates["frame_by_frame"]), "frame_by_frame_fps_max": max(rates["frame_by_frame"]),
           "same_checksum": checks["pipelined"] == checks["frame_by_frame"]}
    row["pipelined_over_frame_by_frame"] = row["pipelined_fps_median"] / row["frame_by_frame_fps_median"]
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
    dev = torch.device("cuda:0")
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    results = kernel_only(args, dev, lut)
    if not args.skip_end_to_end:
        results += end_to_end(args, dev, lut)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
