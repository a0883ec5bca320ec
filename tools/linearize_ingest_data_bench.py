"""Time the data-dependent Normalize of the streamed linearization (profiles/linearize_ingest_data.md):

  kernel only   one ct_ingest_extrema_frames launch pair on 16 frames against 16 ct_ingest_extrema calls, and one
                ct_linearize_ingest_data launch against 16 x (ct_ingest_transform_data + ct_linearize_std) -- what the
                frame-by-frame route runs per frame -- on the same device in the same process, the candidates alternating;
  end to end    frames per second of linearize_dataset_generator over pinned 1080p frames, host clock around the whole run.

    python tools/linearize_ingest_data_bench.py [--launches 30] [--warmup 5] [--frames 64] [--repeats 5]
                                                [--only kernels|end-to-end] [--route auto|frame_by_frame]
                                                [--package-root DIR] [--out FILE.json]

``--package-root DIR`` measures the package of another checkout (a worktree of the parent commit, built there): a checkout
without the per-frame entry points times the old candidates alone and takes the route it has, frame by frame, so the same
tool gives the parent's figures on the same box.  ``--route frame_by_frame`` makes ``pipeline_data_route`` decline.

The lists: A = ``[CastTo(float32), Normalize()]``; B = A with a constant stage in front and a per-channel clamp behind,
``[CastTo, Normalize(4095, 64), Normalize(), ClampAlongDims(1, 3 pairs)]`` (``Normalize(255, 16)`` for uint8); both behind
``CvToTorch`` for the raw (F,H,W,3) BGR frames.  LINEAR, 256 points, MULTIPLIER 0.05.  Byte floors, every byte once over
the 8 TB/s HBM peak of the MI355X: the extrema read ``sizeof(T)`` per sample, the fused pass moves ``sizeof(T) + 8``.
Every row is printed as one JSON line as soon as it is measured.
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


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _draw(shape, dtype, dev):
    """Codes up to 4500 (uint16) / 255 (uint8); every frame gets a top of its own so that no two share their constants."""
    gen = torch.Generator(device=dev).manual_seed(1)
    top = 4500 if dtype == torch.uint16 else 255
    x = torch.randint(0, top + 1, shape, dtype=torch.int16 if dtype == torch.uint16 else dtype, device=dev, generator=gen)
    for f in range(shape[0]):
        x[f].clamp_(max=top - f % 16)
    return x.view(torch.uint16) if dtype == torch.uint16 else x


def _chain(T, dtype, which):
    a = [T.CastTo("float32"), T.Normalize()]
    if which == "A":
        return a
    black = T.Normalize(4095, 64) if dtype == torch.uint16 else T.Normalize(255, 16)
    return [a[0], black, a[1], T.ClampAlongDims(1, PAIRS)]


def _cases():
    for dtype in (torch.uint16, torch.uint8):
        for layout in ("nchw", "nhwc_bgr"):
            for which in ("A", "B"):
                yield dtype, layout, which


def _stats(ts, key):
    return {f"{key}_ms_median": statistics.median(ts) * 1e3, f"{key}_ms_min": min(ts) * 1e3, f"{key}_ms_max": max(ts) * 1e3}


def kernel_only(args, dev, lut, ops, T):
    new = hasattr(ops, "ingest_extrema_frames")
    results = []
    n = KERNEL_FRAMES
    for dtype, layout, which in _cases():
        shape = (n, 3, H, W) if layout == "nchw" else (n, H, W, 3)
        x = _draw(shape, dtype, dev)
        ts = ([T.CvToTorch()] if layout != "nchw" else []) + _chain(T, dtype, which)
        plan = T.fusable_ingest_data(x, ts)
        assert plan is not None and plan.layout == layout and plan.step == 1
        kw = dict(std_mode="multiplier", std_value=0.05)
        staged = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
        out = (torch.empty_like(staged), torch.empty_like(staged))
        out2 = (torch.empty_like(staged), torch.empty_like(staged))
        K2 = torch.empty((n, 4), dtype=torch.float32, device=dev)

        def extrema_per_frame():
            for f in range(n):
                K2[f].copy_(ops.ingest_extrema(x[f:f + 1], plan.prefix, layout, plan.min_val, plan.max_val))

        def extrema_calls_only():  # without the 16-byte copies that only this tool needs
            for f in range(n):
                ops.ingest_extrema(x[f:f + 1], plan.prefix, layout, plan.min_val, plan.max_val)

        def two_launches_per_frame():
            for f in range(n):
                ops.ingest_transform(x[f:f + 1], plan.stages, layout=layout, out=staged[f:f + 1], consts=K2[f])
                ops.linearize_frames(staged[f:f + 1], lut, "linear", out=(out2[0][f:f + 1], out2[1][f:f + 1]), **kw)

        extrema_per_frame()
        two_launches_per_frame()
        row = {"case": f"{n}x3x{H}x{W} {str(dtype).split('.')[-1]} {layout} list {which}", "elements": x.numel()}
        candidates = {"extrema_16_calls": extrema_calls_only, "two_launches_x16": two_launches_per_frame}
        if new:
            K = torch.empty((n, 4), dtype=torch.float32, device=dev)
            ws = ops.ingest_extrema_frames_workspace(n, dev)

            def extrema_frames():
                ops.ingest_extrema_frames(x, plan.prefix, layout, plan.min_val, plan.max_val, out=K, workspace=ws)

            def fused():
                ops.linearize_ingest_frames(x, plan.stages, lut, "linear", layout=layout, out=out, consts=K, **kw)

            extrema_frames()
            fused()
            row["differing"] = int((K.view(torch.int32) != K2.view(torch.int32)).sum()) + \
                int((out[0].view(torch.int32) != out2[0].view(torch.int32)).sum()) + \
                int((out[1].view(torch.int32) != out2[1].view(torch.int32)).sum())
            candidates = {"extrema_frames": extrema_frames, "extrema_16_calls": extrema_calls_only, "fused": fused,
                          "two_launches_x16": two_launches_per_frame}
        times = {k: [] for k in candidates}
        for _ in range(args.launches):  # alternate the candidates: all see the same neighbours and clocks
            for k, fn in candidates.items():
                times[k].append(_time(fn))
        for k in candidates:
            row.update(_stats(times[k][args.warmup:], k))
        row["launches"] = args.launches - args.warmup
        ext_bytes, fused_bytes = x.numel() * x.element_size(), x.numel() * (x.element_size() + 8)
        row.update({"extrema_floor_bytes": ext_bytes, "extrema_floor_ms_at_8TBps": ext_bytes / HBM_PEAK * 1e3,
                    "fused_floor_bytes": fused_bytes, "fused_floor_ms_at_8TBps": fused_bytes / HBM_PEAK * 1e3})
        if new:
            row["extrema_16_calls_over_frames"] = row["extrema_16_calls_ms_median"] / row["extrema_frames_ms_median"]
            row["extrema_frames_TBps"] = ext_bytes / row["extrema_frames_ms_median"] / 1e9
            row["two_launches_x16_over_fused"] = row["two_launches_x16_ms_median"] / row["fused_ms_median"]
            row["fused_floor_TBps"] = fused_bytes / row["fused_ms_median"] / 1e9
        results.append(row)
        print(json.dumps(row), flush=True)
        del x, staged, out, out2
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
    """frames / s of linearize_dataset_generator for the lists on pinned 1080p frames, by the route ``--route`` names."""
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    n = args.frames
    model = ICRFModelDirect(icrf=lut.cpu(), interpolation_mode=InterpMode.LINEAR).to(dev)
    has_route = hasattr(linearization, "pipeline_data_route")
    routes = ["frame_by_frame"] if args.route == "frame_by_frame" or not has_route else ["pipelined", "frame_by_frame"]
    decide = getattr(linearization, "pipeline_data_route", None)
    results = []
    for dtype in (torch.uint16, torch.uint8):
        for layout in ("nchw", "nhwc_bgr"):
            shape = (n, 3, H, W) if layout == "nchw" else (n, H, W, 3)
            codes = _draw(shape, dtype, dev).cpu().pin_memory()
            times = [float(k + 1) for k in range(n)]
            if layout == "nchw":
                ds = StackDataset(codes, times, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                                  materialize_std=False)
            else:
                ds = _raw_frames_dataset(codes, times)
            for which in ("A", "B"):
                ts = ([T.CvToTorch()] if layout != "nchw" else []) + _chain(T, dtype, which)

                def run(route):
                    if has_route:
                        linearization.pipeline_data_route = decide if route == "pipelined" else \
                            (lambda probe, plan, has_dark: "frame_by_frame")
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
                        if has_route:
                            linearization.pipeline_data_route = decide

                rates, checks = {r: [] for r in routes}, {}
                for rep in range(args.repeats + 1):  # the first round warms the routes up
                    for route in routes:
                        fps, checks[route] = run(route)
                        if rep:
                            rates[route].append(fps)
                row = {"case": f"end to end, {n} pinned frames 3x{H}x{W} {str(dtype).split('.')[-1]} {layout} list {which}",
                       "repeats": args.repeats, "package_has_data_route": has_route}
                for route in routes:
                    row.update({f"{route}_fps_median": statistics.median(rates[route]), f"{route}_fps_min": min(rates[route]),
                                f"{route}_fps_max": max(rates[route]), f"{route}_fps_runs": rates[route]})
                if len(routes) == 2:
                    row["same_checksum"] = checks["pipelined"] == checks["frame_by_frame"]
                    row["pipelined_over_frame_by_frame"] = row["pipelined_fps_median"] / row["frame_by_frame_fps_median"]
                results.append(row)
                print(json.dumps(row), flush=True)
            del ds, codes
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("kernels", "end-to-end"), default=None)
    ap.add_argument("--route", choices=("auto", "frame_by_frame"), default="auto")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
    assert args.repeats >= 3, "the spread is taken over at least three runs"
    sys.path.insert(0, os.path.abspath(args.package_root))
    from clair_torch_amd import ops
    from clair_torch_amd.common import transforms as T
    print(json.dumps({"package": os.path.dirname(os.path.abspath(ops.__file__)),
                      "per_frame_entry_points": hasattr(ops, "ingest_extrema_frames")}), flush=True)
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
            json.dump({"package_root": os.path.abspath(args.package_root), "rows": results}, fh, indent=1)


if __name__ == "__main__":
    main()
