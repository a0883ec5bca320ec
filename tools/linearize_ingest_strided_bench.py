"""Time StridedDownscale lists on the streamed linearization (profiles/linearize_ingest_strided.md):

  kernel only   one ct_linearize_ingest_strided launch on 16 raw 1080p uint16 frames against the pair it replaces,
                ct_strided_downscale followed by ct_linearize_ingest on the compacted frames, on the same device in the same
                process, the candidates alternating; every sample is ``--batch`` launches between two device events;
  end to end    frames per second of linearize_dataset_generator over pinned 1080p frames with the downscale in the list,
                by the pipelined route and by the frame-by-frame route (``pipeline_route`` made to decline), host clock around
                the whole run.

    python tools/linearize_ingest_strided_bench.py [--samples 30] [--warmup 5] [--batch 20] [--frames 256] [--repeats 5]
                                                   [--only kernels|end-to-end] [--out FILE.json]

The list: ``[CastTo(float32), Normalize(4095, 64), ClampAlongDims(1, 3 pairs), StridedDownscale(step)]``, behind ``CvToTorch``
for the raw (F,H,W,3) BGR frames; steps 2 and 4.  LINEAR, 256 points, MULTIPLIER 0.05.  Byte floor over the 8 TB/s HBM peak of
the MI355X: the selected source rows at full width (step * pixel bytes is below a 128-byte line) plus 8 bytes written per
output sample; the pair moves the compacted copy twice on top of that.  Every row is printed as one JSON line as soon as it is
measured.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch.utils.data import DataLoader

HBM_PEAK = 8.0e12  # bytes / s
PAIRS = [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)]
KERNEL_FRAMES = 16
H, W = 1080, 1920
STEPS = (2, 4)


def _time(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / batch


def _draw(shape, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    return torch.randint(0, 4501, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)


def _chain(T, layout, step):
    lead = [T.CvToTorch()] if layout != "nchw" else []
    return lead + [T.CastTo("float32"), T.Normalize(4095, 64), T.ClampAlongDims(1, PAIRS), T.StridedDownscale(step)]


def _stats(ts, key):
    return {f"{key}_ms_median": statistics.median(ts) * 1e3, f"{key}_ms_min": min(ts) * 1e3, f"{key}_ms_max": max(ts) * 1e3}


def kernel_only(args, dev, lut, ops, T):
    results = []
    n = KERNEL_FRAMES
    for layout in ("nchw", "nhwc_bgr"):
        shape = (n, 3, H, W) if layout == "nchw" else (n, H, W, 3)
        x = _draw(shape, dev)
        for step in STEPS:
            plan = T.fusable_ingest(x, _chain(T, layout, step))
            assert plan is not None and plan.layout == layout and plan.step == step
            ho, wo = -(-H // step), -(-W // step)
            kw = dict(std_mode="multiplier", std_value=0.05, layout=layout)
            small = torch.empty(ops.downscaled_shape(shape, step, layout), dtype=torch.uint16, device=dev)
            out = tuple(torch.empty((n, 3, ho, wo), dtype=torch.float32, device=dev) for _ in range(2))
            out2 = tuple(torch.empty_like(out[0]) for _ in range(2))

            def strided():
                ops.linearize_ingest_frames_strided(x, step, plan.stages, lut, "linear", out=out, **kw)

            def pair():
                ops.strided_downscale(x, step, layout, out=small)
                ops.linearize_ingest_frames(small, plan.stages, lut, "linear", out=out2, **kw)

            strided()
            pair()
            row = {"case": f"{n}x3x{H}x{W} uint16 {layout} step {step}", "source_elements": x.numel(),
                   "output_samples": out[0].numel(),
                   "differing": int((out[0].view(torch.int32) != out2[0].view(torch.int32)).sum()) +
                   int((out[1].view(torch.int32) != out2[1].view(torch.int32)).sum())}
            candidates = {"strided": strided, "pair": pair}
            times = {k: [] for k in candidates}
            for _ in range(args.samples):  # alternate the candidates: both see the same neighbours and clocks
                for k, fn in candidates.items():
                    times[k].append(_time(fn, args.batch))
            for k in candidates:
                row.update(_stats(times[k][args.warmup:], k))
            row["samples"], row["launches_per_sample"] = args.samples - args.warmup, args.batch
            rows_read = n * 3 * ho * W * 2            # selected source rows at full width, uint16
            written = out[0].numel() * 8
            compact = out[0].numel() * 2              # the compacted copy: written once, read once by the pair
            row.update({"floor_bytes": rows_read + written, "floor_ms_at_8TBps": (rows_read + written) / HBM_PEAK * 1e3,
                        "pair_bytes": rows_read + written + 2 * compact})
            row["pair_over_strided"] = row["pair_ms_median"] / row["strided_ms_median"]
            row["strided_floor_TBps"] = row["floor_bytes"] / row["strided_ms_median"] / 1e9
            row["strided_share_of_floor"] = row["floor_ms_at_8TBps"] / row["strided_ms_median"]
            results.append(row)
            print(json.dumps(row), flush=True)
            del small, out, out2
        del x
        torch.cuda.empty_cache()
    return results


def _raw_frames_dataset(frames, times):
    """(H,W,3) BGR frames as an OpenCV reader hands them over (StackDataset itself insists on (N,C,H,W))."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset

    class RawFrames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, times
            self.files, self.std_hint = list(range(len(times))), ("multiplier", 0.05)
            self.missing_std_mode, self.materialize_std = MissingStdMode.MULTIPLIER, False

        def __len__(self):
            return len(self.exposure_times)

    return RawFrames()


def end_to_end(args, dev, lut, T):
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    n = args.frames
    model = ICRFModelDirect(icrf=lut.cpu(), interpolation_mode=InterpMode.LINEAR).to(dev)
    decide = linearization.pipeline_route
    routes = ["pipelined", "frame_by_frame"]
    results = []
    for layout in ("nchw", "nhwc_bgr"):
        shape = (n, 3, H, W) if layout == "nchw" else (n, H, W, 3)
        codes = torch.cat([_draw((16,) + shape[1:], dev).cpu().view(torch.int16) for _ in range(n // 16)]).view(torch.uint16).pin_memory()
        times = [float(k + 1) for k in range(n)]
        if layout == "nchw":
            ds = StackDataset(codes, times, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
        else:
            ds = _raw_frames_dataset(codes, times)
        for step in STEPS:
            ts = _chain(T, layout, step)

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
                    assert count == n
                    return count / (time.perf_counter() - t0), check
                finally:
                    linearization.pipeline_route = decide

            rates, checks = {r: [] for r in routes}, {}
            for rep in range(args.repeats + 1):  # the first round warms the routes up
                for route in routes:
                    fps, checks[route] = run(route)
                    if rep:
                        rates[route].append(fps)
            row = {"case": f"end to end, {n} pinned frames 3x{H}x{W} uint16 {layout} step {step}", "repeats": args.repeats}
            for route in routes:
                row.update({f"{route}_fps_median": statistics.median(rates[route]), f"{route}_fps_min": min(rates[route]),
                            f"{route}_fps_max": max(rates[route])})
            row["same_checksum"] = checks["pipelined"] == checks["frame_by_frame"]
            row["pipelined_over_frame_by_frame"] = row["pipelined_fps_median"] / row["frame_by_frame_fps_median"]
            results.append(row)
            print(json.dumps(row), flush=True)
        del ds, codes
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("kernels", "end-to-end"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.samples - args.warmup >= 25 and args.repeats >= 3 and args.frames % 16 == 0
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from clair_torch_amd import ops
    from clair_torch_amd.common import transforms as T
    dev = torch.device("cuda:0")
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    results = []
    if args.only != "end-to-end":
        results += kernel_only(args, dev, lut, ops, T)
    if args.only != "kernels":
        results += end_to_end(args, dev, lut, T)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"rows": results}, fh, indent=1)


if __name__ == "__main__":
    main()
