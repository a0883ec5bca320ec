"""Time ct_hdr_merge_dark_ingest_batches against the pair it replaces (profiles/merge_dark_ingest.md is written from its output).

    python tools/merge_dark_ingest_bench.py --out profiles/merge_dark_ingest.json [--exposures 32 --height 4096 --width 4096]

One merge of ``--exposures`` frames of 3 x H x W, LINEAR with Gaussian weights, in batches of 4 and of 8, at 1 and at 8 batches
per launch.  fused: ``ops.hdr_merge_dark_ingest_batches`` on the raw frames.  pair: ``ops.ingest_transform`` per batch into a
float32 stack, then ``ops.hdr_merge_dark_batch`` (1 per launch) or ``ops.hdr_merge_dark_batches`` (8 per launch) -- unchanged
code, timed in the same process.  Per cell: 3 warm-up merges, then ``--runs`` (>= 10) timed ones of each, alternating, with
device events around the whole merge; min / median / max, the ratio of the medians, whether EVERY fused run beat EVERY pair run
(the rule the default of ``compute_hdr_image(fused_dark_ingest=...)`` follows), and the number of result elements whose bits
differ (must be 0).  The constants of a data-dependent Normalize are computed once, outside the timed region, for both.
A shared dark field carries no dark std (one shared dark field with its std for several frames is refused by every route)."""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402

CELLS = [
    # name, dtype, layout, stages, raw std
    ("uint16 planar, black level, MULTIPLIER", torch.uint16, "nchw", [("affine", 64.0, 65535.0 - 64.0, 1.0, 0.0)], "multiplier"),
    ("uint8 planar, black level, MULTIPLIER", torch.uint8, "nchw", [("affine", 4.0, 255.0 - 4.0, 1.0, 0.0)], "multiplier"),
    ("uint16 planar, black level, explicit std", torch.uint16, "nchw", [("affine", 64.0, 65535.0 - 64.0, 1.0, 0.0)], "explicit"),
    ("uint16 BGR behind CvToTorch, MULTIPLIER", torch.uint16, "nhwc_bgr", [("affine", 0.0, 65535.0, 1.0, 0.0)], "multiplier"),
    ("float32 planar, clamp, MULTIPLIER", torch.float32, "nchw", [("clamp", [(0.02, 0.98)])], "multiplier"),
    ("uint16 planar, data-dependent Normalize(), MULTIPLIER", torch.uint16, "nchw", [("affine_data", 1.0, 0.0)], "multiplier"),
]


def make_frames(n, h, w, dtype, layout, dev, gen):
    t = torch.tensor([0.002 * 2.0 ** (k % 8) for k in range(n)], dtype=torch.float64)
    e = torch.rand((3, h, w), device=dev, generator=gen) * (2.0 / float(torch.sqrt(t.min() * t.max())))
    frames = torch.empty((n, 3, h, w) if layout == "nchw" else (n, h, w, 3), dtype=dtype, device=dev)
    for k in range(n):
        x = (e * float(t[k])).clamp_(0, 1).pow_(1 / 2.2)
        if layout != "nchw":
            x = x.flip(0).permute(1, 2, 0)
        if dtype == torch.uint16:   # (through int16: the low 16 bits are the code)
            x = (x * 65535.0).round_().to(torch.int32).to(torch.int16).contiguous().view(torch.uint16)
        elif dtype == torch.uint8:
            x = (x * 255.0).round_().to(torch.uint8)
        frames[k] = x
    return frames, t


def timed(fn, runs_a, runs_b, fn_b, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(n):
        for f, runs in ((fn, runs_a), (fn_b, runs_b)):
            start.record()
            f()
            stop.record()
            stop.synchronize()
            runs.append(start.elapsed_time(stop))


def stats(runs):
    return dict(min_ms=min(runs), median_ms=statistics.median(runs), max_ms=max(runs), runs=len(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exposures", type=int, default=32)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 10:
        raise SystemExit("--runs must be at least 10")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    n, h, w = a.exposures, a.height, a.width
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (1.8, 2.2, 2.6)]).to(dev)
    dark = 0.1 * torch.rand((n, 3, h, w), device=dev, generator=gen)
    dark_std = 0.002 + 0.01 * torch.rand((n, 3, h, w), device=dev, generator=gen)
    sd = 0.002 + 0.03 * torch.rand((n, 3, h, w), device=dev, generator=gen)
    kw = dict(lut=lut, interp="linear", gaussian_weight=True, reference_order=False)
    results = []
    for name, dtype, layout, stages, std_mode in CELLS:
        frames, t = make_frames(n, h, w, dtype, layout, dev, gen)
        for dark_kind in ("per frame", "shared"):
            for bsz in (4, 8):
                cuts = [slice(k, k + bsz) for k in range(0, n, bsz)]
                fb, tb = [frames[c] for c in cuts], [t[c].to(dev) for c in cuts]
                darks = [dark[c] if dark_kind == "per frame" else dark[:1] for c in cuts]
                dstds = [dark_std[c] for c in cuts] if dark_kind == "per frame" else None
                stds = [sd[c] for c in cuts] if std_mode == "explicit" else None
                skw = {} if std_mode == "explicit" else dict(std_mode=std_mode, std_value=0.05)
                consts = [ops.ingest_extrema(f, [], layout, None, None) for f in fb] if stages[0][0] == "affine_data" else None
                pick = lambda v, s: None if v is None else v[s]   # noqa: E731
                for per_launch in (1, 8):
                    groups = [slice(k, k + per_launch) for k in range(0, len(cuts), per_launch)]
                    out = {}

                    def fused():
                        st = ops.MergeState((3, h, w), dev, dstds is not None)
                        for g in groups:
                            r = ops.hdr_merge_dark_ingest_batches(fb[g], stages, tb[g], darks[g], pick(dstds, g), consts=pick(consts, g),
                                                                  stds=pick(stds, g), layout=layout, state=st, finalize=g is groups[-1],
                                                                  **skw, **kw)
                        out["fused"] = r

                    def pair():
                        st = ops.MergeState((3, h, w), dev, dstds is not None)
                        for g in groups:
                            idx = range(len(cuts))[g]
                            x32 = [ops.ingest_transform(fb[i], stages, layout, consts=None if consts is None else consts[i]) for i in idx]
                            if per_launch == 1:
                                i = idx[0]
                                r = ops.hdr_merge_dark_batch(x32[0], tb[i], darks[i], None if dstds is None else dstds[i],
                                                             std=None if stds is None else stds[i], state=st, finalize=g is groups[-1],
                                                             **skw, **kw)
                            else:
                                r = ops.hdr_merge_dark_batches(x32, tb[g], darks[g], pick(dstds, g), stds=pick(stds, g), state=st,
                                                               finalize=g is groups[-1], **skw, **kw)
                        out["pair"] = r

                    timed(fused, [], [], pair, 3)
                    fr, pr = [], []
                    timed(fused, fr, pr, pair, a.runs)
                    diff = int((out["fused"][0] != out["pair"][0]).sum())
                    if out["fused"][1] is not None:
                        diff += int((out["fused"][1] != out["pair"][1]).sum())
                    row = dict(cell=name, dark=dark_kind, batch=bsz, batches_per_launch=per_launch, fused=stats(fr), pair=stats(pr),
                               ratio_of_medians=statistics.median(fr) / statistics.median(pr), every_fused_run_faster=max(fr) < min(pr),
                               differing_elements=diff)
                    results.append(row)
                    print(json.dumps(row), flush=True)
                    del out
        del frames
        torch.cuda.empty_cache()
    doc = dict(shape=[n, 3, h, w], interp="linear", weights="gauss", device=torch.cuda.get_device_name(0), results=results,
               every_cell_every_run_faster=all(r["every_fused_run_faster"] for r in results),
               differing_elements=sum(r["differing_elements"] for r in results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "results"}))


if __name__ == "__main__":
    main()
