"""Time ct_ingest_extrema_frames + ct_linearize_dark_ingest_data against the four launches they replace -- ct_ingest_extrema_frames,
ct_ingest_transform_data into a planar float32 stack, ct_dark_field_blur into xb and sigma_eff, the float32 explicit-uncertainty
ct_linearize_std -- on the same device in the same process, and linearize_dataset_generator end to end with
``fused_dark_ingest_data`` on and off (profiles/linearize_dark_ingest_data.md).  The method is that of
tools/linearize_dark_ingest_bench.py, whose helpers this script imports.

    python tools/linearize_dark_ingest_data_bench.py [--launches 30] [--warmup 5] [--runs 5] [--frames 64] [--height 1080]
                                                     [--width 1920] [--out FILE.json] [--md FILE.md]

Kernel cases, one group of 16 x 3 x H x W frames behind the data-dependent Normalize alone (``Normalize()``), one matched dark
field (and its std) per frame, 256 points: uint16 raw (H,W,3) BGR frames with MULTIPLIER 0.05, LINEAR; uint16 planar likewise;
uint8 BGR; uint16 planar with an explicit std stack; uint16 BGR, CATMULL.  The fused pair is ONE ct_ingest_extrema_frames call
and ONE ct_linearize_dark_ingest_data launch.  The four launches are this build's own, timed at their best: the extrema of the 16
frames in one call (the same kernel), the blur and the linearization ONE launch each on the 16 frames; only
ct_ingest_transform_data runs per frame, 16 launches, because it takes one set of constants per call.  Device-event time of every
run, the candidates alternating, median / min / max after warm-up.  Bytes moved are counted from the shapes: per sample the
extrema pass reads sizeof(T); the fused launch reads sizeof(T) + 8 (+ 4 explicit) and writes 8; the other three read sizeof(T)
and write 4, read 4 + 8 (+ 4) and write 8, read 8 and write 8.  The outputs of the two routes are compared bit for bit
(``differing`` must be 0).

End to end: ``--frames`` uint16 frames in pinned host memory, MULTIPLIER uncertainties, one dark field on the host; raw BGR
frames behind [CvToTorch, CastTo, Normalize()] and planar frames behind [CastTo, Normalize()].  The generator is consumed frame
by frame (nothing is kept) and the host clock stops after the last frame; ``fused_dark_ingest_data=False`` is the frame-by-frame
route -- the route of the parent commit for these lists --, the two alternate, fused first, as in the parent profiles.
``every_fused_run_faster`` of BOTH rows is the rule for a later flip of the default of
``linearize_dataset_generator(fused_dark_ingest_data=...)``.
"""
import argparse
import json
import os
import sys
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402
from linearize_dark_bench import FRAMES, HBM_PEAK, _draw, _stats, _time  # noqa: E402

# (dtype, raw BGR frames, std mode, interpolation)
CASES = [(torch.uint16, True, "multiplier", "linear"), (torch.uint16, False, "multiplier", "linear"),
         (torch.uint8, True, "multiplier", "linear"), (torch.uint16, False, "explicit", "linear"),
         (torch.uint16, True, "multiplier", "catmull")]
STAGES = [("affine_data", 1.0, 0.0)]


def bytes_moved(f, c, h, w, elem, explicit):
    """(fused pair, four launches) bytes, every byte once; the extrema pass (sizeof(T) per sample) is in both."""
    samples = f * c * h * w
    extra = 4 if explicit else 0
    return samples * (elem + (elem + 8 + extra + 8)), samples * (elem + (elem + 4) + (4 + 8 + extra + 8) + (8 + 8))


def kernel_cases(args, dev, lut):
    rows = []
    f, c, h, w = FRAMES, 3, args.height, args.width
    for dtype, raw, std_mode, interp in CASES:
        gen = torch.Generator(device=dev).manual_seed(1)
        x = _draw((f, h, w, c) if raw else (f, c, h, w), dtype, dev, gen)
        layout = "nhwc_bgr" if raw else "nchw"
        dark = 0.1 * torch.rand((f, c, h, w), device=dev, generator=gen)   # straddles the 0.05 threshold
        dark_std = 0.002 + 0.01 * torch.rand((f, c, h, w), device=dev, generator=gen)
        sd = (0.002 + 0.03 * torch.rand((f, c, h, w), device=dev, generator=gen)) if std_mode == "explicit" else None
        src = dict(std=sd) if sd is not None else dict(std_mode="multiplier", std_value=0.05)
        darks, dark_stds = list(dark), list(dark_std)
        outs = (torch.empty((f, c, h, w), device=dev), torch.empty((f, c, h, w), device=dev))
        consts, ws = torch.empty((f, 4), device=dev), ops.ingest_extrema_frames_workspace(f, dev)   # a ring slot's own buffers
        px = torch.empty((f, c, h, w), device=dev)
        got = {}

        def fused():
            K = ops.ingest_extrema_frames(x, (), layout, out=consts, workspace=ws)
            got["fused"] = ops.linearize_dark_ingest_frames_data(x, STAGES, darks, dark_stds, lut, interp, consts=K, layout=layout,
                                                                 out=outs, **src)

        def four():
            K = ops.ingest_extrema_frames(x, (), layout, out=consts, workspace=ws)
            for k in range(f):
                ops.ingest_transform(x[k:k + 1], STAGES, layout, out=px[k:k + 1], consts=K[k])
            xb, sig = ops.dark_field_blur(px, dark, dark_std, **src)
            got["four"] = ops.linearize_frames(xb, lut, interp, std=sig)

        fused()
        four()
        differing = sum(int((got["fused"][k].view(torch.int32) != got["four"][k].view(torch.int32)).sum()) for k in (0, 1))
        times = {"fused": [], "four": []}
        for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
            times["fused"].append(_time(fused))
            times["four"].append(_time(four))
        fb, tb = bytes_moved(f, c, h, w, x.element_size(), sd is not None)
        row = {"case": f"{'x'.join(map(str, x.shape))} {str(dtype).split('.')[-1]} {'BGR' if raw else 'planar'} Normalize() {std_mode} {interp}",
               "launches": args.launches - args.warmup, "differing": differing, "fused_bytes": fb, "four_bytes": tb,
               "bytes_ratio": fb / tb, "fused_floor_ms_at_8TBps": fb / HBM_PEAK * 1e3}
        for name, ts in times.items():
            row.update({f"{name}_{k}": v for k, v in _stats(ts[args.warmup:]).items()})
        row["fused_over_four"] = row["fused_ms_median"] / row["four_ms_median"]
        row["fused_TBps"] = fb / (row["fused_ms_median"] * 1e-3) / 1e12
        row["four_TBps"] = tb / (row["four_ms_median"] * 1e-3) / 1e12
        row["fused_faster_beyond_spread"] = row["fused_ms_max"] < row["four_ms_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, dark, dark_std, sd, got, darks, dark_stds, outs, px
        torch.cuda.empty_cache()
    return rows


def end_to_end(args, dev, lut, raw):
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    n, c, h, w = args.frames, 3, args.height, args.width
    gen = torch.Generator().manual_seed(2)
    shape = (n, h, w, c) if raw else (n, c, h, w)
    codes = torch.randint(-32768, 32768, shape, dtype=torch.int16, generator=gen).view(torch.uint16).pin_memory()
    ds = StackDataset(codes, [1.0] * n, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
    art = ArtefactStack(0.1 * torch.rand((c, h, w), generator=gen), 0.002 + 0.01 * torch.rand((c, h, w), generator=gen))
    model = ICRFModelDirect(icrf=lut.cpu(), interpolation_mode=InterpMode.LINEAR).to(dev)
    tf = ([CvToTorch()] if raw else []) + [CastTo("float32"), Normalize()]
    sums = {}

    def run(flag, check=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total = 0.0
        for lin, lsd, _ in linearize_dataset_generator(loader, "cuda", model, dark_field_dataset=art, fused_dark_ingest_data=flag,
                                                       gpu_transforms=tf):
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
    what = "raw BGR (H,W,3) behind CvToTorch + CastTo + Normalize()" if raw else "planar behind CastTo + Normalize()"
    row = {"case": f"linearize_dataset_generator {n} x 3x{h}x{w} uint16 {what}, multiplier linear, pinned host frames",
           "runs": args.runs, "digests_equal": sums[True] == sums[False]}
    for flag, name in ((True, "fused"), (False, "frame_by_frame")):
        row.update({f"{name}_{k}": v for k, v in _stats([n / t for t in times[flag]], 1.0, "fps").items()})
        row[f"{name}_seconds"] = times[flag]
    row["fused_over_frame_by_frame_fps"] = row["fused_fps_median"] / row["frame_by_frame_fps_median"]
    row["every_fused_run_faster"] = max(times[True]) < min(times[False])
    print(json.dumps(row), flush=True)
    return row


def markdown(results):
    head, rows, e2e = results[0], results[1:-2], results[-2:]
    verdict = all(r["every_fused_run_faster"] for r in e2e)
    lines = ["## Measured", "",
             f"Device: {head['device']}.  Written by `tools/linearize_dark_ingest_data_bench.py`; the numbers are in",
             "`linearize_dark_ingest_data.json`.", "",
             "Device-event time per group of 16 frames: the fused pair (ct_ingest_extrema_frames + ct_linearize_dark_ingest_data) / the four",
             "launches (ct_ingest_extrema_frames, 16 x ct_ingest_transform_data, ct_dark_field_blur and the float32 ct_linearize_std on the 16",
             f"frames), the two alternating, median [min .. max] of {rows[0]['launches']} runs after warm-up.  Bytes are counted from the shapes.", "",
             "| case | fused pair ms | four launches ms | fused / four | bytes fused / four | fused TB/s | four TB/s | differing bits | faster beyond spread |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['fused_ms_median']:.3f} [{r['fused_ms_min']:.3f} .. {r['fused_ms_max']:.3f}] | "
                     f"{r['four_ms_median']:.3f} [{r['four_ms_min']:.3f} .. {r['four_ms_max']:.3f}] | {r['fused_over_four']:.3f} | "
                     f"{r['bytes_ratio']:.3f} | {r['fused_TBps']:.2f} | {r['four_TBps']:.2f} | {r['differing']} | "
                     f"{'yes' if r['fused_faster_beyond_spread'] else 'no'} |")
    lines += ["", "End to end (host clock from the first `next()` to the last frame and a synchronise; frames in pinned host memory, consumed",
              f"frame by frame; {e2e[0]['runs']} runs each, alternating, after one warm-up run each), frames / s:", "",
              "| case | fused_dark_ingest_data=True | fused_dark_ingest_data=False (frame by frame, the parent's route) | ratio | outputs agree | every fused run faster |",
              "|---|---|---|---|---|---|"]
    for r in e2e:
        lines.append(f"| {r['case']} | {r['fused_fps_median']:.1f} [{r['fused_fps_min']:.1f} .. {r['fused_fps_max']:.1f}] | "
                     f"{r['frame_by_frame_fps_median']:.1f} [{r['frame_by_frame_fps_min']:.1f} .. {r['frame_by_frame_fps_max']:.1f}] | "
                     f"{r['fused_over_frame_by_frame_fps']:.2f} | {'yes' if r['digests_equal'] else 'NO'} | "
                     f"{'yes' if r['every_fused_run_faster'] else 'no'} |")
    lines += ["", "The rule for a later flip of the default of `linearize_dataset_generator(fused_dark_ingest_data=...)`, set before measuring:",
              "True only if every fused run is faster than every frame-by-frame run in BOTH rows.  Verdict of this measurement:",
              f"**the rule {'is met' if verdict else 'is NOT met'}**.  The default stays `False` in this change whatever the verdict: the",
              "route is opt-in, and changing a default is a decision of its own.", ""]
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
    results += [end_to_end(args, dev, lut, True), end_to_end(args, dev, lut, False)]
    for path, text in ((args.out, json.dumps(results, indent=1)), (args.md, markdown(results))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)


if __name__ == "__main__":
    main()
