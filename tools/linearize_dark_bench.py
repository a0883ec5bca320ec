"""Time ct_linearize_dark against the two launches it replaces -- ct_dark_field_blur into float32 stacks xb and sigma_eff, then
the float32 explicit-uncertainty ct_linearize_std on them -- on the same device in the same process, and
linearize_dataset_generator end to end with ``fused_dark`` on and off (profiles/linearize_dark.md).

    python tools/linearize_dark_bench.py [--launches 30] [--warmup 5] [--runs 5] [--frames 64] [--height 1080] [--width 1920]
                                         [--out FILE.json] [--md FILE.md]

The pair is this build's own: neither of its two kernels is touched by the fused one, which lives in a file of its own.  It
is timed at its best: ONE ct_dark_field_blur launch on the 16 frames with their 16 dark fields (the same bits as 16 launches of
one frame) and ONE ct_linearize_std launch.  Cases: 16 x 3 x H x W planar frames, one matched dark field (and its std) per
frame, 256 points; uint16 and uint8 codes with MULTIPLIER 0.05, uint16 codes with an explicit std stack, float32 pixels with
MULTIPLIER 0.05, LINEAR, and uint16 MULTIPLIER with CATMULL.  Device-event time of every run, the candidates alternating,
median / min / max after warm-up.  Bytes moved are counted from the shapes: per sample the fused launch reads sizeof(T) + 8
(+ 4 explicit) and writes 8; the pair reads sizeof(T) + 8 (+ 4), writes 8, reads 8 again and writes 8.  The outputs of the two
routes are also compared (``differing`` must be 0).

End to end: ``--frames`` uint16 frames in pinned host memory behind CastTo + Normalize(65535, 0), MULTIPLIER uncertainties, one
dark field on the host; the generator is consumed frame by frame (nothing is kept) and the host clock stops after the last
frame.  ``fused_dark=False`` is the frame-by-frame route untouched by the fused one: the baseline.  The two alternate.
``every_fused_run_faster`` is the rule behind the default of ``linearize_dataset_generator(fused_dark=...)``: every fused run
faster than every frame-by-frame run.
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

HBM_PEAK = 8.0e12  # bytes / s
CASES = [(torch.uint16, "multiplier", "linear"), (torch.uint8, "multiplier", "linear"), (torch.uint16, "explicit", "linear"),
         (torch.float32, "multiplier", "linear"), (torch.uint16, "multiplier", "catmull")]
FRAMES = 16


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _draw(shape, dtype, dev, gen):
    if dtype == torch.uint16:  # torch draws no uint16: all 65 536 codes through the int16 view
        return torch.randint(-32768, 32768, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    if dtype == torch.float32:
        return torch.rand(shape, device=dev, generator=gen)
    return torch.randint(0, 256, shape, dtype=dtype, device=dev, generator=gen)


def bytes_moved(f, c, h, w, elem, explicit):
    """(fused, pair) bytes per launch(es), every byte once."""
    samples = f * c * h * w
    read = elem + 8 + (4 if explicit else 0)
    return samples * (read + 8), samples * (read + 8 + 16)


def _stats(ts, unit=1e3, name="ms"):
    return {f"{name}_median": statistics.median(ts) * unit, f"{name}_min": min(ts) * unit, f"{name}_max": max(ts) * unit}


def kernel_cases(args, dev, lut):
    rows = []
    f, c, h, w = FRAMES, 3, args.height, args.width
    for dtype, std_mode, interp in CASES:
        gen = torch.Generator(device=dev).manual_seed(1)
        x = _draw((f, c, h, w), dtype, dev, gen)
        dark = 0.1 * torch.rand((f, c, h, w), device=dev, generator=gen)   # straddles the 0.05 threshold
        dark_std = 0.002 + 0.01 * torch.rand((f, c, h, w), device=dev, generator=gen)
        sd = (0.002 + 0.03 * torch.rand((f, c, h, w), device=dev, generator=gen)) if std_mode == "explicit" else None
        top = {torch.uint16: 65535.0, torch.uint8: 255.0}.get(dtype)
        src = dict(std=sd) if sd is not None else dict(std_mode="multiplier", std_value=0.05)
        darks, dark_stds = list(dark), list(dark_std)
        outs = (torch.empty((f, c, h, w), device=dev), torch.empty((f, c, h, w), device=dev))
        got = {}

        def fused():
            got["fused"] = ops.linearize_dark_frames(x, darks, dark_stds, lut, interp, max_code=top, out=outs, **src)

        def pair():
            xb, sig = ops.dark_field_blur(x, dark, dark_std, max_code=top, **src)
            got["pair"] = ops.linearize_frames(xb, lut, interp, std=sig)

        fused()
        pair()
        differing = sum(int((got["fused"][k].view(torch.int32) != got["pair"][k].view(torch.int32)).sum()) for k in (0, 1))
        times = {"fused": [], "pair": []}
        for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
            times["fused"].append(_time(fused))
            times["pair"].append(_time(pair))
        fb, pb = bytes_moved(f, c, h, w, x.element_size(), sd is not None)
        row = {"case": f"{f}x{c}x{h}x{w} {str(dtype).split('.')[-1]} {std_mode} {interp}", "launches": args.launches - args.warmup,
               "differing": differing, "fused_bytes": fb, "pair_bytes": pb, "bytes_ratio": fb / pb,
               "fused_floor_ms_at_8TBps": fb / HBM_PEAK * 1e3}
        for name, ts in times.items():
            row.update({f"{name}_{k}": v for k, v in _stats(ts[args.warmup:]).items()})
        row["fused_over_pair"] = row["fused_ms_median"] / row["pair_ms_median"]
        row["fused_TBps"] = fb / (row["fused_ms_median"] * 1e-3) / 1e12
        row["pair_TBps"] = pb / (row["pair_ms_median"] * 1e-3) / 1e12
        row["fused_faster_beyond_spread"] = row["fused_ms_max"] < row["pair_ms_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, dark, dark_std, sd, got, darks, dark_stds, outs
        torch.cuda.empty_cache()
    return rows


def end_to_end(args, dev, lut):
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    n, c, h, w = args.frames, 3, args.height, args.width
    gen = torch.Generator().manual_seed(2)
    codes = torch.randint(-32768, 32768, (n, c, h, w), dtype=torch.int16, generator=gen).view(torch.uint16).pin_memory()
    ds = StackDataset(codes, [1.0] * n, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
    art = ArtefactStack(0.1 * torch.rand((c, h, w), generator=gen), 0.002 + 0.01 * torch.rand((c, h, w), generator=gen))
    model = ICRFModelDirect(icrf=lut.cpu(), interpolation_mode=InterpMode.LINEAR).to(dev)
    sums = {}

    def run(flag, check=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = 0.0
        for lin, lsd, _ in linearize_dataset_generator(loader, "cuda", model, dark_field_dataset=art, fused_dark=flag,
                                                       gpu_transforms=[CastTo("float32"), Normalize(65535, 0)]):
            if check:  # (outside the timed runs) a digest of every frame: the two routes must agree to the bit
                total += float(lin.double().sum()) + float(lsd.double().sum())
        torch.cuda.synchronize()
        if check:
            sums[flag] = total
        return time.perf_counter() - t0

    for flag in (True, False):  # warm-up, with the digest
        run(flag, check=True)
    times = {True: [], False: []}
    for _ in range(args.runs):
        for flag in (True, False):
            times[flag].append(run(flag))
    row = {"case": f"linearize_dataset_generator {n}x{c}x{h}x{w} uint16 multiplier linear, pinned host frames", "runs": args.runs,
           "digests_equal": sums[True] == sums[False]}
    for flag, name in ((True, "fused"), (False, "frame_by_frame")):
        row.update({f"{name}_{k}": v for k, v in _stats([n / t for t in times[flag]], 1.0, "fps").items()})
        row[f"{name}_seconds"] = times[flag]
    row["fused_over_frame_by_frame_fps"] = row["fused_fps_median"] / row["frame_by_frame_fps_median"]
    row["every_fused_run_faster"] = max(times[True]) < min(times[False])
    print(json.dumps(row), flush=True)
    return row


def markdown(results):
    head, rows, e2e = results[0], results[1:-1], results[-1]
    lines = ["# Dark-field blur + linearization in one pass: ct_linearize_dark against the pair it replaces", "",
             f"Device: {head['device']}.  Written by `tools/linearize_dark_bench.py`; the numbers are in `linearize_dark.json`.", "",
             "Device-event time per launch (fused) / per two launches (ct_dark_field_blur on the 16 frames + float32 ct_linearize_std), the",
             f"two alternating, median [min .. max] of {rows[0]['launches']} runs after warm-up.  Bytes are counted from the shapes.", "",
             "| case | fused ms | pair ms | fused / pair | bytes fused / pair | fused TB/s | pair TB/s | differing | faster beyond spread |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['fused_ms_median']:.3f} [{r['fused_ms_min']:.3f} .. {r['fused_ms_max']:.3f}] | "
                     f"{r['pair_ms_median']:.3f} [{r['pair_ms_min']:.3f} .. {r['pair_ms_max']:.3f}] | {r['fused_over_pair']:.3f} | "
                     f"{r['bytes_ratio']:.3f} | {r['fused_TBps']:.2f} | {r['pair_TBps']:.2f} | {r['differing']} | "
                     f"{'yes' if r['fused_faster_beyond_spread'] else 'no'} |")
    lines += ["", "End to end (host clock from the first `next()` to the last frame and a synchronise; frames in pinned host memory, consumed",
              f"frame by frame; {e2e['runs']} runs each, alternating, after one warm-up run each), frames / s:", "",
              "| case | fused_dark=True | fused_dark=False (frame by frame) | ratio | outputs agree | every fused run faster |", "|---|---|---|---|---|---|",
              f"| {e2e['case']} | {e2e['fused_fps_median']:.1f} [{e2e['fused_fps_min']:.1f} .. {e2e['fused_fps_max']:.1f}] | "
              f"{e2e['frame_by_frame_fps_median']:.1f} [{e2e['frame_by_frame_fps_min']:.1f} .. {e2e['frame_by_frame_fps_max']:.1f}] | "
              f"{e2e['fused_over_frame_by_frame_fps']:.2f} | {'yes' if e2e['digests_equal'] else 'NO'} | "
              f"{'yes' if e2e['every_fused_run_faster'] else 'no'} |", "",
              "The rule for the default of `linearize_dataset_generator(fused_dark=...)`, set before measuring: True only if every fused",
              f"run is faster than every frame-by-frame run.  It gives **fused_dark={e2e['every_fused_run_faster']}**.", "",
              "## Not measured, out of scope", "",
              "* Not measured: explicit uncertainty images and float32 frames end to end; other frame sizes; CATMULL end to end; pageable",
              "  host frames; more than one dark field in the run (the device cache was exercised by the tests only); kernel time by",
              "  rocprofv3 (the figures above are device events around the ops fronts, allocation of the pair's two stacks included).",
              "* Out of scope: row bands (no halo is built: the generator has no `tile=`); fused `gpu_transforms` chains or a",
              "  StridedDownscale behind a dark field (they stay frame by frame); reference-pinned dark-field parity (the blur is",
              "  torchvision's, restated in `oracle/eager_torch.py`; the specification here is bit-equality with the pair).", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5, help="timed generator runs per setting (one more warms up)")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
    assert args.runs >= 5, "at least 5 end-to-end runs per setting"
    dev = torch.device("cuda:0")
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    results = [{"device": torch.cuda.get_device_name(dev)}]
    print(json.dumps(results[0]), flush=True)
    results += kernel_cases(args, dev, lut)
    results.append(end_to_end(args, dev, lut))
    for path, text in ((args.out, json.dumps(results, indent=1)), (args.md, markdown(results))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)


if __name__ == "__main__":
    main()
