"""Time ct_hdr_merge_ingest_batch against the two launches it replaces -- ct_ingest_transform into a float32 stack, then the
float32 ct_hdr_merge_batch on that stack -- and against the code-route merge of the same stack (the floor: 2 B per sample
and no chain), on the same device in the same process (profiles/merge_ingest.md).

    python tools/merge_ingest_bench.py [--launches 30] [--warmup 5] [--two-launch-lib PATH/libclair_hip.so] [--out FILE.json]
    python tools/merge_ingest_bench.py --profile 6      (the launches alone, for a counter run: tools/pmc_merge_ingest.sh)

The list is ``[CastTo(float32), Normalize(65535, 256)]`` (``Normalize(255, 16)`` for uint8), behind ``CvToTorch`` for the raw
(B,H,W,3) BGR frames; LINEAR, 256 points, Gaussian weights, MULTIPLIER 0.05; the code route runs ``Normalize(65535, 0)``.
``--two-launch-lib``: take the two launches from another build of the library (the parent commit's), loaded beside this
one.  Device-event time of every run, the candidates alternating, median / min / max after warm-up; the byte floor is
``B * sizeof(T)`` read and 12 written per output element, every byte once, over the 8 TB/s HBM peak of the MI355X.  The
outputs of the fused launch and of the two launches are also compared (``differing`` must be 0).  The power state --
performance level, shader / memory clocks and socket power as ``rocm-smi`` reports them (read only) -- is noted before the
first and right after the last launch of every case.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import _native as nv  # noqa: E402
from clair_torch_amd import ops  # noqa: E402
from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize, plan_staging  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
CASES = [((32, 3, 4096, 4096), torch.uint16, ("nchw", "nhwc_bgr")), ((64, 3, 1080, 1920), torch.uint8, ("nchw", "nhwc_bgr"))]


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _power_state():
    """Performance level, clocks and power as rocm-smi prints them (a read-only query in a child process)."""
    try:
        out = subprocess.run(["rocm-smi", "--showperflevel", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.SubprocessError) as err:
        return [f"rocm-smi unavailable: {err}"]
    keep = ("Performance Level", "sclk", "mclk", "Power")
    return [" ".join(line.split()) for line in out.splitlines() if line.startswith("GPU[0]") and any(k in line for k in keep)]


def _draw(shape, dtype, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    if dtype == torch.uint16:  # torch draws no uint16: all 65 536 codes through the int16 view
        return torch.randint(-32768, 32768, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    return torch.randint(0, 256, shape, dtype=dtype, device=dev, generator=gen)


def _two_launches(lib, x, arr, n_stages, layout, staged, expo, lut, mean_out, std_out, dev):
    """ct_ingest_transform + the float32 ct_hdr_merge_batch of ``lib`` (this build's, or another one's)."""
    b, c, h, w = staged.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.ct_ingest_transform(p(x), nv.DTYPE_U16 if x.dtype == torch.uint16 else nv.DTYPE_U8, ops._LAYOUT[layout], b, c, h * w, arr,
                                 n_stages, p(staged), stream)
    assert rc == 0, rc
    geom = nv.Geometry(channels=c, h_tile=h, width=w, h_global=h, row_offset=0, image_stride=c * h * w, layout=nv.LAYOUT_NCHW)
    icrf = nv.Icrf(lut_dev=lut.data_ptr(), n_points=lut.shape[1], interp=nv.INTERP_LINEAR)
    rc = lib.ct_hdr_merge_batch(p(staged), nv.DTYPE_F32, 1.0, b, ctypes.byref(geom), None, nv.STD_MULTIPLIER, 0.05, p(expo),
                                ctypes.byref(icrf), nv.WEIGHT_GAUSS, None, None, None, p(mean_out), p(std_out),
                                nv.MERGE_FIRST_BATCH | nv.MERGE_FINALIZE, stream)
    assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--two-launch-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0, help="run each candidate of the C2 cases this many times and stop (no timing)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.profile or args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
    dev = torch.device("cuda:0")
    here = nv.load()
    other = here
    if args.two_launch_lib:
        other = ctypes.CDLL(os.path.abspath(args.two_launch_lib))
        for name in ("ct_ingest_transform", "ct_hdr_merge_batch"):
            getattr(other, name).argtypes = getattr(here, name).argtypes
            getattr(other, name).restype = ctypes.c_int32
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]).to(dev)
    results = [{"device": torch.cuda.get_device_name(dev), "two_launch_lib": args.two_launch_lib or "this build"}]
    print(json.dumps(results[0]), flush=True)
    for (b, c, h, w), dtype, layouts in (CASES[:1] if args.profile else CASES):
        top, black = (65535, 256) if dtype == torch.uint16 else (255, 16)
        expo = torch.tensor([0.001 * 2.0 ** (k * 0.25) for k in range(b)], dtype=torch.float64, device=dev)
        for layout in layouts:
            x = _draw((b, c, h, w) if layout == "nchw" else (b, h, w, c), dtype, dev)
            lead = [CvToTorch()] if layout != "nchw" else []
            plan = plan_staging(x, lead + [CastTo("float32"), Normalize(top, black)])
            assert plan.route == "ingest" and plan.source_layout == layout
            arr, n_stages = ops._ingest_stages(plan.stages, c)
            staged = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
            mean2 = torch.empty((c, h, w), dtype=torch.float64, device=dev)
            std2 = torch.empty((c, h, w), dtype=torch.float32, device=dev)
            kw = dict(lut=lut, interp="linear", gaussian_weight=True, std_mode="multiplier", std_value=0.05)
            got = {}

            def fused():
                got["fused"] = ops.hdr_merge_ingest_batch(x, plan.stages, expo, layout=layout, **kw)

            def two_launches():
                _two_launches(other, x, arr, n_stages, layout, staged, expo, lut, mean2, std2, dev)

            def code_route():
                got["code"] = ops.hdr_merge_batch(x, expo, max_code=float(top), layout=layout, **kw)

            if args.profile:
                for _ in range(args.profile):
                    fused()
                    two_launches()
                    code_route()
                torch.cuda.synchronize()
                continue
            power = {"before": _power_state()}
            fused()
            two_launches()
            code_route()
            differing = int((got["fused"][0].view(torch.int64) != mean2.view(torch.int64)).sum()) + \
                int((got["fused"][1].view(torch.int32) != std2.view(torch.int32)).sum())
            times = {"fused": [], "two_launch": [], "code_route": []}
            for _ in range(args.launches):  # alternate the candidates: all see the same neighbours and clocks
                times["fused"].append(_time(fused))
                times["two_launch"].append(_time(two_launches))
                times["code_route"].append(_time(code_route))
            power["after"] = _power_state()
            floor_bytes = c * h * w * (b * x.element_size() + 12)
            row = {"case": f"{b}x{c}x{h}x{w} {str(dtype).split('.')[-1]} {layout}", "launches": args.launches - args.warmup,
                   "floor_bytes": floor_bytes, "floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3, "differing": differing, "power_state": power}
            for name, ts in times.items():
                ts = ts[args.warmup:]
                row.update({f"{name}_ms_median": statistics.median(ts) * 1e3, f"{name}_ms_min": min(ts) * 1e3, f"{name}_ms_max": max(ts) * 1e3})
            row["two_launch_over_fused"] = row["two_launch_ms_median"] / row["fused_ms_median"]
            row["fused_share_of_floor"] = row["floor_ms_at_8TBps"] / row["fused_ms_median"]
            results.append(row)
            print(json.dumps(row), flush=True)
            del x, staged, mean2, std2, got
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
