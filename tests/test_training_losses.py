"""l1_loss and ssim of gs2mesh_amd.training (GS/utils/loss_utils.py) on the CPU: definitions, identities, and ssim against a
direct-sum statement of the same formula written here (unfold + explicit weighted sums, no conv2d)."""
import math

import numpy as np
import torch

from gs2mesh_amd.training import l1_loss, ssim


def pair(seed=0, H=40, W=48):
    """a textured image and a distorted copy of it, [3,H,W] in [0,1]"""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(0.7 * x + c) * np.cos(0.45 * y - c) for c in range(3)])
    a = np.clip(base + r.normal(0, 0.05, base.shape), 0, 1)
    b = np.clip(0.9 * base + 0.03 + r.normal(0, 0.08, base.shape), 0, 1)
    return torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)


def ssim_statement(a, b, dtype):
    """mean SSIM by direct sums in ``dtype``: 11 x 11 Gaussian window (sigma 1.5, normalised in 1-D, outer product), zero
    padding 5, local moments as weighted sums over the window, C1 = 0.01^2, C2 = 0.03^2"""
    a, b = a.to(dtype), b.to(dtype)
    g = torch.tensor([math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)], dtype=dtype)
    g = g / g.sum()
    w = (g[:, None] * g[None, :]).reshape(1, 121, 1)
    C, H, W = a.shape

    def local(x):       # [C,H,W] -> weighted window sum at every pixel
        cols = torch.nn.functional.unfold(x[:, None], kernel_size=11, padding=5)        # [C, 121, H*W]
        return (cols * w).sum(dim=1).reshape(C, H, W)

    mu1, mu2 = local(a), local(b)
    s11 = local(a * a) - mu1 * mu1
    s22 = local(b * b) - mu2 * mu2
    s12 = local(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return float(m.mean())


def test_l1_loss_is_the_mean_absolute_difference():
    a, b = pair()
    want = float(np.abs(a.numpy().astype(np.float64) - b.numpy().astype(np.float64)).mean())
    assert abs(float(l1_loss(a, b)) - want) <= 1e-6 * want
    assert float(l1_loss(a, a)) == 0.0


def test_ssim_identities():
    a, b = pair()
    assert abs(float(ssim(a, a)) - 1.0) <= 4 * np.finfo(np.float32).eps
    assert abs(float(ssim(a, b)) - float(ssim(b, a))) <= 4 * np.finfo(np.float32).eps
    assert 0.0 < float(ssim(a, b)) < 0.95
    batch = ssim(torch.stack([a, b]), torch.stack([b, b]), size_average=False)
    assert batch.shape == (2,) and abs(float(batch[1]) - 1.0) <= 4 * np.finfo(np.float32).eps
    assert abs(float(batch[0]) - float(ssim(a, b))) <= 4 * np.finfo(np.float32).eps


def test_ssim_equals_the_direct_sum_statement():
    """bound (the rule of test_raster_backward.py): 4 x the difference between the statement in fp32 and in fp64"""
    a, b = pair()
    s64, s32 = ssim_statement(a, b, torch.float64), ssim_statement(a, b, torch.float32)
    got = float(ssim(a, b))
    print(f"ssim {got:.9f}  statement fp64 {s64:.9f}  fp32 {s32:.9f}  |got - s64| {abs(got - s64):.3e}  "
          f"|s32 - s64| {abs(s32 - s64):.3e}")
    assert abs(got - s64) <= 4 * abs(s32 - s64)
