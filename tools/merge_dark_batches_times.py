"""Time one ct_hdr_merge_dark_batches call against the same batches through k calls of ct_hdr_merge_dark_batch of ANOTHER build of
the library (``--parent-lib``: libclair_hip.so built from the parent commit, with or without the entry point under test), and
beside it the per-batch path of this build.

    python tools/merge_dark_batches_times.py --parent-lib /path/to/parent/libclair_hip.so --out profiles/merge_dark_batches.json

Workload: the shape of profiles/merge_dark.md (3 x 4096 x 4096 frames), 32 exposures as 8 batches of 4 and as 4 batches of 8, LINEAR +
Gaussian weights; uint16 MULTIPLIER, uint8 MULTIPLIER, uint16 explicit std and float32 (MULTIPLIER); one dark field per frame with
its std, and one shared dark field (without a dark std: a shared one with its std is refused for more than one frame).  Same
process, same buffers; the variants alternate within every repetition, the first repetitions are discarded, device events around
``--inner`` whole merges per sample.  Every variant's outputs are compared bit for bit before anything is timed."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import _native as nv  # noqa: E402


def bind(path):
    lib = ctypes.CDLL(path)
    lib.ct_hdr_merge_dark_batch.restype = ctypes.c_int32
    lib.ct_hdr_merge_dark_batch.argtypes = nv.load().ct_hdr_merge_dark_batch.argtypes
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--shape", type=int, nargs=3, default=[3, 4096, 4096])
    ap.add_argument("--exposures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    new, parent = nv.load(), bind(args.parent_lib)
    c, h, w = args.shape
    n = args.exposures
    gen = torch.Generator(device=dev).manual_seed(1)
    geom = nv.Geometry(channels=c, h_tile=h, width=w, h_global=h, row_offset=0, image_stride=c * h * w, layout=nv.LAYOUT_NCHW)
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (1.8, 2.2, 2.6)])[:c].contiguous().to(dev)
    icrf = nv.Icrf(lut_dev=lut.data_ptr(), n_points=256, interp=nv.INTERP_LINEAR)
    expo = torch.tensor([0.002 * 2.0 ** (k % 8) for k in range(n)], dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    results = []
    configs = [("uint16 MULTIPLIER", torch.uint16, nv.STD_MULTIPLIER), ("uint8 MULTIPLIER", torch.uint8, nv.STD_MULTIPLIER),
               ("uint16 explicit std", torch.uint16, nv.STD_EXPLICIT), ("float32 MULTIPLIER", torch.float32, nv.STD_MULTIPLIER)]
    for name, dtype, std_mode in configs:
        top = {torch.uint16: 65535.0, torch.uint8: 255.0, torch.float32: 1.0}[dtype]
        if dtype == torch.float32:
            frames = torch.rand((n, c, h, w), generator=gen, device=dev)
        elif dtype == torch.uint8:
            frames = torch.randint(0, 256, (n, c, h, w), generator=gen, device=dev, dtype=torch.uint8)
        else:   # uniform 16-bit codes
            frames = torch.randint(-32768, 32768, (n, c, h, w), generator=gen, device=dev, dtype=torch.int16).view(torch.uint16)
        sd = (0.002 + 0.03 * torch.rand((n, c, h, w), generator=gen, device=dev)) if std_mode == nv.STD_EXPLICIT else None
        for dark_kind in ("per frame + std", "shared, no std"):
            per_frame = dark_kind.startswith("per")
            dark = 0.1 * torch.rand((n if per_frame else 1, c, h, w), generator=gen, device=dev)
            dark_std = (0.002 + 0.01 * torch.rand(dark.shape, generator=gen, device=dev)) if per_frame else None
            with_var = dark_std is not None
            state = [torch.empty((c, h, w), dtype=torch.float64, device=dev), torch.empty((c, h, w), dtype=torch.float32, device=dev),
                     torch.empty((c, h, w), dtype=torch.float32, device=dev)]
            outs = {k: (torch.empty((c, h, w), dtype=torch.float64, device=dev), torch.empty((c, h, w), dtype=torch.float32, device=dev))
                    for k in ("parent", "multi", "per_batch")}
            for size in (4, 8):
                k = n // size
                cuts = [(b * size, (b + 1) * size) for b in range(k)]
                dk = lambda a, b: dark[a:b] if per_frame else dark  # noqa: E731

                def per_batch(lib, out):
                    for i, (a, b) in enumerate(cuts):
                        flags = (nv.MERGE_FIRST_BATCH if i == 0 else 0) | (nv.MERGE_FINALIZE if i == k - 1 else 0)
                        rc = lib.ct_hdr_merge_dark_batch(p(frames[a:b]), DT[dtype], top, size,
                                                         ctypes.byref(geom), None, p(None if sd is None else sd[a:b]), std_mode, 0.05,
                                                         p(dk(a, b)), p(None if dark_std is None else dark_std[a:b]), size if per_frame else 1,
                                                         0.05, 50.0, p(expo[a:b]), ctypes.byref(icrf), nv.WEIGHT_GAUSS, p(state[0]), p(state[1]),
                                                         p(state[2]), p(out[0]), p(out[1]), flags, stream)
                        assert rc == 0, rc

                arr = lambda ts: (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
                stack_arr = arr([frames[a:b] for a, b in cuts])
                std_arr = arr([sd[a:b] for a, b in cuts]) if sd is not None else None
                dark_arr = arr([dk(a, b) for a, b in cuts])
                dark_std_arr = arr([None if dark_std is None else dark_std[a:b] for a, b in cuts])
                sizes = (ctypes.c_int32 * k)(*[size] * k)
                dark_sizes = (ctypes.c_int32 * k)(*[size if per_frame else 1] * k)

                def multi(out):
                    rc = new.ct_hdr_merge_dark_batches(stack_arr, sizes, k, DT[dtype], top, ctypes.byref(geom), None, std_arr, std_mode, 0.05,
                                                       dark_arr, dark_std_arr, dark_sizes, 0.05, 50.0, p(expo), ctypes.byref(icrf),
                                                       nv.WEIGHT_GAUSS, None, None, None, p(out[0]), p(out[1]),
                                                       nv.MERGE_FIRST_BATCH | nv.MERGE_FINALIZE | nv.MERGE_REQUIRE_ONE_LAUNCH, stream)
                    assert rc == 0, rc

                variants = {"parent": lambda: per_batch(parent, outs["parent"]), "multi": lambda: multi(outs["multi"]),
                            "per_batch": lambda: per_batch(new, outs["per_batch"])}
                for fn in variants.values():
                    fn()
                torch.cuda.synchronize(dev)
                for other in ("multi", "per_batch"):   # faster and different is not faster
                    assert torch.equal(outs[other][0], outs["parent"][0]), (name, dark_kind, size, other)
                    assert not with_var or torch.equal(outs[other][1], outs["parent"][1]), (name, dark_kind, size, other)
                times = {v: [] for v in variants}
                for rep in range(args.warmup + args.reps):
                    for v, fn in variants.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.inner):
                            fn()
                        e1.record()
                        e1.synchronize()
                        if rep >= args.warmup:
                            times[v].append(e0.elapsed_time(e1) / args.inner)
                row = dict(config=name, dark=dark_kind, batches=k, batch_size=size,
                           **{v: dict(min_ms=min(t), max_ms=max(t), median_ms=sorted(t)[len(t) // 2]) for v, t in times.items()})
                row["ratio_multi_over_parent"] = row["multi"]["median_ms"] / row["parent"]["median_ms"]
                row["multi_wins_every_run"] = row["multi"]["max_ms"] < row["parent"]["min_ms"]
                results.append(row)
                print(json.dumps(row), flush=True)
            del dark, dark_std, state, outs
        del frames, sd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(shape=args.shape, exposures=n, reps=args.reps, warmup=args.warmup, inner=args.inner, device=torch.cuda.get_device_name(0),
                       rows=results), f, indent=1)


DT = {torch.uint8: nv.DTYPE_U8, torch.uint16: nv.DTYPE_U16, torch.float32: nv.DTYPE_F32}

if __name__ == "__main__":
    main()
