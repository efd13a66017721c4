"""tests/loss_statement.py (the numpy f32 statement of gs2m_photo_loss_forward / _backward) against the reference's formulas:
``training.loss_fn`` / ``training.ssim`` evaluated in fp64 on CPU torch, autograd for the gradient.  The margin is torch's own
f32 evaluation of the same functions on the same inputs: the statement's largest error on the SSIM map and on the gradient
is at most twice the f32 torch path's, per input.  CPU only; the kernels are compared with the statement bit for bit in
test_photo_loss.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_statement
from gs2mesh_amd import training

LAMBDA = 0.2


def noise():
    r = np.random.default_rng(0)
    return r.uniform(0, 1, (3, 37, 53)).astype(np.float32), r.uniform(0, 1, (3, 37, 53)).astype(np.float32)


def ramps():
    r = np.random.default_rng(1)
    v, u = np.meshgrid(np.linspace(0, 1, 48), np.linspace(0, 1, 40))
    base = np.stack([u, v, 0.5 * (u + v)])
    return ((base + r.normal(0, 0.01, base.shape)).astype(np.float32),
            (base[:, ::-1] * 0.8 + 0.1 + r.normal(0, 0.01, base.shape)).astype(np.float32))


def tiny():
    r = np.random.default_rng(2)
    return r.uniform(0, 1, (3, 4, 7)).astype(np.float32), r.uniform(0, 1, (3, 4, 7)).astype(np.float32)


def near_identical():
    r = np.random.default_rng(3)
    v, u = np.meshgrid(np.linspace(0, 1, 96), np.linspace(0, 1, 80))
    y = np.stack([0.5 + 0.4 * np.sin(6 * u) * np.cos(5 * v), u * v, 0.3 + 0.5 * u]).astype(np.float32)
    return (y + r.normal(0, 1e-3, y.shape).astype(np.float32)).astype(np.float32), y


INPUTS = {"noise_3x37x53": noise, "ramps_3x40x48": ramps, "tiny_3x4x7": tiny, "near_identical_3x80x96": near_identical}


def torch_map(img1, img2):
    """the ssim_map of training.ssim (which returns its mean only), in the dtype of its arguments"""
    channel = img1.size(-3)
    w = training._window(11, channel, img1)
    conv = lambda x: F.conv2d(x, w, padding=5, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(img1 * img1) - mu1_sq
    sigma2_sq = conv(img2 * img2) - mu2_sq
    sigma12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def torch_eval(x, y, dtype):
    a = torch.from_numpy(x).to(dtype).requires_grad_(True)
    b = torch.from_numpy(y).to(dtype)
    loss = training.loss_fn(a, b, LAMBDA)
    loss.backward()
    with torch.no_grad():
        m = torch_map(a, b)
        assert abs(float(m.mean()) - float(training.ssim(a, b))) <= 1e-6
    return m.double().numpy(), a.grad.double().numpy(), float(loss.detach())


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_statement_is_as_close_to_fp64_as_torch_f32(name):
    x, y = INPUTS[name]()
    map64, grad64, loss64 = torch_eval(x, y, torch.float64)
    map32, grad32, loss32 = torch_eval(x, y, torch.float32)
    fw = loss_statement.forward(x, y)
    grad = loss_statement.backward(x, y, fw, LAMBDA, 1.0)
    e_map, t_map = np.abs(fw["map"] - map64).max(), np.abs(map32 - map64).max()
    e_grad, t_grad = np.abs(grad - grad64).max(), np.abs(grad32 - grad64).max()
    (loss, _, _), _ = loss_statement.scalars64(fw, LAMBDA)
    print(f"{name}: map error {e_map:.3e} (torch f32 {t_map:.3e}), gradient error {e_grad:.3e} (torch f32 {t_grad:.3e}), "
          f"largest |gradient| {np.abs(grad64).max():.3e}, N {x.size}, loss error {abs(loss - loss64):.3e} "
          f"(torch f32 {abs(loss32 - loss64):.3e})")
    assert e_map <= 2 * t_map
    assert e_grad <= 2 * t_grad
    # the loss is affine in the mean of the map, and |x - y| is one f32 rounding from exact
    assert abs(loss - loss64) <= LAMBDA * 2 * t_map + 2.0 ** -23


def test_identical_images_give_exactly_one_and_zero():
    x, _ = noise()
    fw = loss_statement.forward(x, x.copy())
    assert np.all(fw["map"] == np.float32(1.0))
    assert not fw["absdiff"].any()
    (loss, l1, ssim), _ = loss_statement.scalars64(fw, LAMBDA)
    assert l1 == 0.0 and abs(ssim - 1.0) < 1e-7 and abs(loss) < 1e-7


def test_window_is_the_reference_window_to_f32_rounding():
    w = loss_statement.window()
    ref = training._window(11, 1, torch.zeros(1))[0, 0].numpy()
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-7
    assert np.abs(np.outer(w, w) - ref).max() <= 2 ** -24 * ref.max() * 4
