"""Scenes for the fused dark-field tests (test_gpu_merge_dark.py, test_gpu_linearize_dark.py): one recipe for both."""
import numpy as np
import torch


def scene(seed, n, c, h, w, period=None):
    """A consistent exposure series through a gamma curve (exposure times doubling, starting over every ``period`` frames if
    given), uncertainties, one dark field PER FRAME straddling the 0.05 threshold (so a wrong pointer or frame stride shows)
    with its std, and a LUT whose rows differ."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.tensor([0.002 * 2.0 ** (k % period if period else k) for k in range(n)], dtype=torch.float64)
    e = torch.rand((c, h, w), generator=gen, dtype=torch.float64) * (2.0 / float(torch.sqrt(t.min() * t.max())))
    x = ((e.unsqueeze(0) * t.view(-1, 1, 1, 1)).clamp(0, 1) ** (1 / 2.2)).float()
    sd = (0.002 + 0.03 * torch.rand(x.shape, generator=gen)).float()
    dark = (0.1 * torch.rand((n, c, h, w), generator=gen)).float()
    dark_std = (0.002 + 0.01 * torch.rand((n, c, h, w), generator=gen)).float()
    lut = torch.stack([torch.linspace(0, 1, 256) ** p for p in (1.8, 2.2, 2.6)])[:c].contiguous()
    return x, sd, t, dark, dark_std, lut


def as_dtype(x, dtype):
    """(stack of that dtype, max_code)"""
    if dtype == torch.float32:
        return x, None
    top = 65535 if dtype == torch.uint16 else 255
    return torch.from_numpy(np.rint(x.numpy().astype(np.float64) * top).astype(np.uint16 if top == 65535 else np.uint8)), float(top)
