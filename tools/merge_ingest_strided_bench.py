"""Time ct_hdr_merge_ingest_strided_batches against the two launches it replaces -- ct_strided_downscale of every batch into a
compacted copy, then ct_hdr_merge_ingest_batch(es) on the copies -- on the same device in the same process
(profiles/merge_ingest_strided.md).

    python tools/merge_ingest_strided_bench.py [--runs 30] [--warmup 5] [--exposures 32] [--height 4096] [--width 4096]
                                               [--out FILE.json] [--md FILE.md]

The pair is this build's own and untouched: ct_downscale.hip, ct_merge_ingest.hip and ct_merge_ingest_multi.hip compile to the
instructions they had before the strided kernels existed (the note records the diff).  A run is one whole merge of
``--exposures`` exposures of 3 x H x W in batches of 4, LINEAR, 256 points, Gaussian weights:

  one per launch     every batch a call of its own, the streaming state in memory in between
                     (pair: strided_downscale + hdr_merge_ingest_batch per batch; fused: hdr_merge_ingest_batch_strided per batch)
  eight per launch   what compute_hdr_image queues: all batches in one call, the state in registers
                     (pair: strided_downscale per batch, then one hdr_merge_ingest_batches; fused: one hdr_merge_ingest_batches_strided)

at steps 2 and 4, for uint16 planar frames behind a black level, uint8 planar, uint16 BGR frames behind CvToTorch, uint16 planar
with explicit uncertainties (of the downscaled shape), and a data-dependent Normalize in front of the downscale (the extrema
pass is the same on both sides and outside the timed region).  Device-event time of every run, the candidates alternating,
median / min / max after warm-up.  Bytes are counted from the shapes: per output sample and exposure the pair reads the selected
rows at full width (step x sizeof(T)), writes sizeof(T) and reads it again; the fused launch reads the selected rows only; both
add 4 B with explicit uncertainties and 12 B of outputs per element (one per launch: 32 B of state per element and batch more,
on both sides).  ``fused_faster_beyond_spread`` says that the slowest fused run was faster than the fastest pair: the rule behind
the default of ``compute_hdr_image(fused_downscale=...)`` asks for that in every row.  The outputs of the two routes are also
compared bit by bit (``differing`` must be 0).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
BATCH = 4
STEPS = (2, 4)
# name, dtype, layout, explicit std, data-dependent Normalize
CASES = [("uint16 planar black level", torch.uint16, "nchw", False, False),
         ("uint8 planar black level", torch.uint8, "nchw", False, False),
         ("uint16 BGR behind CvToTorch", torch.uint16, "nhwc_bgr", False, False),
         ("uint16 planar explicit std", torch.uint16, "nchw", True, False),
         ("uint16 planar Normalize() in front", torch.uint16, "nchw", False, True)]


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _draw(shape, dtype, dev, gen):
    if dtype == torch.uint16:  # torch draws no uint16: 10-bit codes on a black level through the int16 view
        return torch.randint(32, 1101, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    return torch.randint(0, 256, shape, dtype=dtype, device=dev, generator=gen)


def bytes_moved(n, c, ho, wo, step, elem, explicit):
    """(fused, pair) bytes of one merge, every byte once, state traffic left out."""
    samples, outputs = n * c * ho * wo, c * ho * wo
    extra = 4 if explicit else 0
    return samples * (step * elem + extra) + outputs * 12, samples * (step * elem + 2 * elem + extra) + outputs * 12


def _stats(ts):
    return {"ms_median": statistics.median(ts) * 1e3, "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3}


def _differing(a, b):
    return int((a[0].view(torch.int64) != b[0].view(torch.int64)).sum()) + int((a[1].view(torch.int32) != b[1].view(torch.int32)).sum())


def cases(args, dev, lut):
    rows = []
    c, h, w, n = 3, args.height, args.width, args.exposures
    k = n // BATCH
    expo = torch.tensor([0.001 * 2.0 ** (i * 0.25) for i in range(n)], dtype=torch.float64, device=dev)
    expos = [expo[b * BATCH:(b + 1) * BATCH] for b in range(k)]
    for name, dtype, layout, explicit, data in CASES:
        gen = torch.Generator(device=dev).manual_seed(1)
        shape = (BATCH, c, h, w) if layout == "nchw" else (BATCH, h, w, c)
        frames = [_draw(shape, dtype, dev, gen) for _ in range(k)]
        if data:
            stages = [("affine_data", 1.0, 0.0)]
            consts = [ops.ingest_extrema(f, (), layout) for f in frames]   # of the full batch: the Normalize stands in front
        else:
            stages, consts = [("affine", 16.0, 184.0, 1.0, 0.0) if dtype == torch.uint8 else ("affine", 64.0, 959.0, 1.0, 0.0)], None
        for step in STEPS:
            ho, wo = -(-h // step), -(-w // step)
            stds = [0.002 + 0.03 * torch.rand((BATCH, c, ho, wo), device=dev, generator=gen) for _ in range(k)] if explicit else None
            kw = dict(lut=lut, interp="linear", gaussian_weight=True, layout=layout)
            if not explicit:
                kw.update(std_mode="multiplier", std_value=0.05)
            item = lambda lst, b: None if lst is None else lst[b]   # noqa: E731
            for per_launch in (1, k):
                got = {}

                def fused():
                    if per_launch == k:
                        got["fused"] = ops.hdr_merge_ingest_batches_strided(frames, step, stages, expos, stds=stds, consts=consts, **kw)
                        return
                    state = ops.MergeState((c, ho, wo), dev, True)
                    for b in range(k):
                        got["fused"] = ops.hdr_merge_ingest_batch_strided(frames[b], step, stages, expos[b], std=item(stds, b),
                                                                         consts=item(consts, b), state=state, finalize=b == k - 1, **kw)

                def pair():
                    if per_launch == k:
                        small = [ops.strided_downscale(f, step, layout) for f in frames]
                        got["pair"] = ops.hdr_merge_ingest_batches(small, stages, expos, stds=stds, consts=consts, **kw)
                        return
                    state = ops.MergeState((c, ho, wo), dev, True)
                    for b in range(k):
                        small = ops.strided_downscale(frames[b], step, layout)
                        got["pair"] = ops.hdr_merge_ingest_batch(small, stages, expos[b], std=item(stds, b), consts=item(consts, b),
                                                                 state=state, finalize=b == k - 1, **kw)

                fused()
                pair()
                differing = _differing(got["fused"], got["pair"])
                times = {"fused": [], "pair": []}
                for _ in range(args.runs):  # alternate the candidates: both see the same neighbours and clocks
                    times["fused"].append(_time(fused))
                    times["pair"].append(_time(pair))
                fb, pb = bytes_moved(n, c, ho, wo, step, frames[0].element_size(), explicit)
                row = {"case": f"{n}x{c}x{h}x{w} {name}", "step": step, "batches_per_launch": per_launch, "runs": args.runs - args.warmup,
                       "differing": differing, "fused_bytes": fb, "pair_bytes": pb, "bytes_ratio": fb / pb,
                       "fused_floor_ms_at_8TBps": fb / HBM_PEAK * 1e3}
                for side, ts in times.items():
                    row.update({f"{side}_{key}": v for key, v in _stats(ts[args.warmup:]).items()})
                row["fused_over_pair"] = row["fused_ms_median"] / row["pair_ms_median"]
                row["fused_TBps"] = fb / (row["fused_ms_median"] * 1e-3) / 1e12
                row["pair_TBps"] = pb / (row["pair_ms_median"] * 1e-3) / 1e12
                row["fused_faster_beyond_spread"] = row["fused_ms_max"] < row["pair_ms_min"]
                rows.append(row)
                print(json.dumps(row), flush=True)
                del got
            del stds
            torch.cuda.empty_cache()
        del frames
        torch.cuda.empty_cache()
    return rows


def markdown(results):
    head, rows = results[0], results[1:]
    lines = [f"Device: {head['device']}.  Written by `tools/merge_ingest_strided_bench.py`.", "",
             "Device-event time of one whole merge, fused (ct_hdr_merge_ingest_strided_batches) against the pair (ct_strided_downscale of",
             "every batch + ct_hdr_merge_ingest_batch(es)), the two alternating, median [min .. max] of "
             f"{rows[0]['runs']} runs after warm-up.", "Bytes are counted from the shapes.", "",
             "| case | step | batches / launch | fused ms | pair ms | fused / pair | bytes fused / pair | fused TB/s | pair TB/s | differing | faster beyond spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['step']} | {r['batches_per_launch']} | "
                     f"{r['fused_ms_median']:.3f} [{r['fused_ms_min']:.3f} .. {r['fused_ms_max']:.3f}] | "
                     f"{r['pair_ms_median']:.3f} [{r['pair_ms_min']:.3f} .. {r['pair_ms_max']:.3f}] | {r['fused_over_pair']:.3f} | "
                     f"{r['bytes_ratio']:.3f} | {r['fused_TBps']:.2f} | {r['pair_TBps']:.2f} | {r['differing']} | "
                     f"{'yes' if r['fused_faster_beyond_spread'] else 'no'} |")
    every = all(r["fused_faster_beyond_spread"] for r in rows)
    same = all(r["differing"] == 0 for r in rows)
    lines += ["", f"Differing bits anywhere: **{'none' if same else 'SOME'}**.",
              f"Fused faster than the pair in every row, beyond the spread: **{'yes' if every else 'no'}**.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--exposures", type=int, default=32)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.exposures % BATCH == 0 and 1 <= args.exposures // BATCH <= ops.MAX_MERGE_BATCHES
    assert args.runs > args.warmup
    dev = torch.device("cuda:0")
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    results = [{"device": torch.cuda.get_device_name(dev)}]
    print(json.dumps(results[0]), flush=True)
    results += cases(args, dev, lut)
    for path, text in ((args.out, json.dumps(results, indent=1)), (args.md, markdown(results))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)


if __name__ == "__main__":
    main()
