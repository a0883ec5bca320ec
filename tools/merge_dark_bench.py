"""Time ct_hdr_merge_dark_batch against the two launches it replaces -- ct_dark_field_blur into float32 stacks xb and sigma_eff,
then the float32 explicit-uncertainty ct_hdr_merge_batch on them -- on the same device in the same process, and
compute_hdr_image end to end with ``fused_dark`` on and off (profiles/merge_dark.md).

    python tools/merge_dark_bench.py [--launches 30] [--warmup 5] [--height 4096] [--width 4096] [--out FILE.json] [--md FILE.md]

The pair is this build's own: neither of its two kernels is touched by the fused one, which lives in a file of its own.
Cases: 3 x H x W planar frames, one matched dark field (and its std) per frame, LINEAR, 256 points, Gaussian weights; uint16
and uint8 codes with MULTIPLIER 0.05 and uint16 codes with an explicit std stack; batches of 4 (the reference's default) and
32.  Device-event time of every run, the candidates alternating, median / min / max after warm-up.  Bytes moved are counted
from the shapes: per sample the fused launch reads sizeof(T) + 8 (+ 4 explicit), the pair reads sizeof(T) + 8 (+ 4), writes 8
and reads 8 again; both write 12 per output element.  ``fused_faster_beyond_spread`` says that the slowest fused launch was
faster than the fastest pair: the criterion behind the default of ``compute_hdr_image(fused_dark=...)``.  The outputs of the
two routes are also compared (``differing`` must be 0).
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
CASES = [(torch.uint16, "multiplier"), (torch.uint8, "multiplier"), (torch.uint16, "explicit")]
BATCHES = (4, 32)


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
    return torch.randint(0, 256, shape, dtype=dtype, device=dev, generator=gen)


def bytes_moved(b, c, h, w, elem, explicit):
    """(fused, pair) bytes per launch(es), every byte once."""
    samples, outputs = b * c * h * w, c * h * w
    read = elem + 8 + (4 if explicit else 0)
    return samples * read + outputs * 12, samples * (read + 16) + outputs * 12


def _stats(ts):
    return {"ms_median": statistics.median(ts) * 1e3, "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3}


def kernel_cases(args, dev, lut):
    rows = []
    c, h, w = 3, args.height, args.width
    for dtype, std_mode in CASES:
        for b in BATCHES:
            gen = torch.Generator(device=dev).manual_seed(1)
            x = _draw((b, c, h, w), dtype, dev, gen)
            dark = 0.1 * torch.rand((b, c, h, w), device=dev, generator=gen)   # straddles the 0.05 threshold
            dark_std = 0.002 + 0.01 * torch.rand((b, c, h, w), device=dev, generator=gen)
            sd = (0.002 + 0.03 * torch.rand((b, c, h, w), device=dev, generator=gen)) if std_mode == "explicit" else None
            expo = torch.tensor([0.001 * 2.0 ** (k * 0.25) for k in range(b)], dtype=torch.float64, device=dev)
            top = 65535.0 if dtype == torch.uint16 else 255.0
            src = dict(std=sd) if sd is not None else dict(std_mode="multiplier", std_value=0.05)
            kw = dict(lut=lut, interp="linear", gaussian_weight=True)
            got = {}

            def fused():
                got["fused"] = ops.hdr_merge_dark_batch(x, expo, dark, dark_std, max_code=top, **src, **kw)

            def pair():
                xb, sig = ops.dark_field_blur(x, dark, dark_std, max_code=top, **src)
                got["pair"] = ops.hdr_merge_batch(xb, expo, std=sig, **kw)

            fused()
            pair()
            differing = int((got["fused"][0].view(torch.int64) != got["pair"][0].view(torch.int64)).sum()) + \
                int((got["fused"][1].view(torch.int32) != got["pair"][1].view(torch.int32)).sum())
            times = {"fused": [], "pair": []}
            for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
                times["fused"].append(_time(fused))
                times["pair"].append(_time(pair))
            fb, pb = bytes_moved(b, c, h, w, x.element_size(), sd is not None)
            row = {"case": f"{b}x{c}x{h}x{w} {str(dtype).split('.')[-1]} {std_mode}", "launches": args.launches - args.warmup,
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
            del x, dark, dark_std, sd, got
            torch.cuda.empty_cache()
    return rows


def end_to_end(args, dev, lut):
    """compute_hdr_image on 8 frames in batches of 4: host frames (the one host-to-device copy per batch included), the dark
    field and its std already on the device; host clock around a call that ends in a synchronise."""
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    n, c, h, w = 8, 3, args.height, args.width
    gen = torch.Generator().manual_seed(2)
    codes = torch.randint(-32768, 32768, (n, c, h, w), dtype=torch.int16, generator=gen).view(torch.uint16)
    expo = [0.001 * 2.0 ** k for k in range(n)]
    ds = StackDataset(codes, expo, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    loader = DataLoader(ds, batch_size=4, shuffle=False, collate_fn=custom_collate)
    dgen = torch.Generator(device=dev).manual_seed(3)
    art = ArtefactStack(0.1 * torch.rand((c, h, w), device=dev, generator=dgen), 0.002 + 0.01 * torch.rand((c, h, w), device=dev, generator=dgen))
    model = ICRFModelDirect(icrf=lut.cpu(), interpolation_mode=InterpMode.LINEAR).to(dev)
    out = {}

    def run(flag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[flag] = compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, dark_field_dataset=art,
                                      gpu_transforms=[CastTo("float32"), Normalize(65535, 0)], fused_dark=flag)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times = {True: [], False: []}
    for _ in range(args.calls + 1):
        for flag in (True, False):
            times[flag].append(run(flag))
    differing = int((out[True][0] != out[False][0]).sum()) + int((out[True][1] != out[False][1]).sum())
    row = {"case": f"compute_hdr_image {n}x{c}x{h}x{w} uint16 multiplier, batches of 4", "calls": args.calls, "differing": differing}
    for flag, name in ((True, "fused"), (False, "pair")):
        row.update({f"{name}_{k}": v for k, v in _stats(times[flag][1:]).items()})
    row["fused_over_pair"] = row["fused_ms_median"] / row["pair_ms_median"]
    print(json.dumps(row), flush=True)
    return row


def markdown(results):
    head, rows, e2e = results[0], results[1:-1], results[-1]
    lines = ["# Dark-field blur + merge in one pass: ct_hdr_merge_dark_batch against the pair it replaces", "",
             f"Device: {head['device']}.  Written by `tools/merge_dark_bench.py`; the numbers are in `merge_dark.json`.", "",
             "Device-event time per launch (fused) / per two launches (ct_dark_field_blur + float32 ct_hdr_merge_batch), the two",
             f"alternating, median [min .. max] of {rows[0]['launches']} runs after warm-up.  Bytes are counted from the shapes.", "",
             "| case | fused ms | pair ms | fused / pair | bytes fused / pair | fused TB/s | pair TB/s | differing | faster beyond spread |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['fused_ms_median']:.3f} [{r['fused_ms_min']:.3f} .. {r['fused_ms_max']:.3f}] | "
                     f"{r['pair_ms_median']:.3f} [{r['pair_ms_min']:.3f} .. {r['pair_ms_max']:.3f}] | {r['fused_over_pair']:.3f} | "
                     f"{r['bytes_ratio']:.3f} | {r['fused_TBps']:.2f} | {r['pair_TBps']:.2f} | {r['differing']} | "
                     f"{'yes' if r['fused_faster_beyond_spread'] else 'no'} |")
    lines += ["", "End to end (host clock around a call that ends in a synchronise; host frames, one host-to-device copy per batch):", "",
              "| case | fused_dark=True ms | fused_dark=False ms | ratio | differing |", "|---|---|---|---|---|",
              f"| {e2e['case']} | {e2e['fused_ms_median']:.1f} [{e2e['fused_ms_min']:.1f} .. {e2e['fused_ms_max']:.1f}] | "
              f"{e2e['pair_ms_median']:.1f} [{e2e['pair_ms_min']:.1f} .. {e2e['pair_ms_max']:.1f}] | {e2e['fused_over_pair']:.3f} | {e2e['differing']} |", ""]
    every = all(r["fused_faster_beyond_spread"] for r in rows)
    lines += [f"Fused faster than the pair at every measured shape, beyond the spread: **{'yes' if every else 'no'}**.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="timed compute_hdr_image calls per setting (one more warms up)")
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
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
