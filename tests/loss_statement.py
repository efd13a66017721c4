"""Plain numpy statement of gs2m_photo_loss_forward / _backward (include/gs2mesh_amd.h, gs2mesh_amd/csrc/loss_kernels.h):
every operation is one float32 operation, in the order the header fixes.

  window    w = f32(g / sum(g)), g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) in double, summed in index order
  filter    F = V(H(.)), zero padding, each 11-tap sum accumulated from zero in index order: acc = acc + w[k] * term
  moments   mu1 = F(x), mu2 = F(y), exx = F(x * x), eyy = F(y * y), exy = F(x * y)
  map       A = (mu1^2 + mu2^2) + C1, B = (s1 + s2) + C2, C = 2 mu1 mu2 + C1, D = 2 s12 + C2, m = (C * D) / (A * B)
  partials  p0 = 2 * ((((mu2 * D) / AB - (mu2 * C) / AB) - (mu1 * m) / A) + (mu1 * m) / B), p1 = -(m / B), p2 = (2 * C) / AB
  gradient  dx = ((F(g * p0) + (2 * x) * F(g * p1)) + y * F(g * p2)) + l * sign(x - y), g = gl * (-kb), l = gl * ka
"""
import math

import numpy as np

R = 5
TAPS = 2 * R + 1
TILE_W, TILE_H = 32, 16                 # LOSS_TW, LOSS_TH
F32 = np.float32
C1 = F32(0.01) * F32(0.01)
C2 = F32(0.03) * F32(0.03)


def chain(planes, H, W):
    """LOSS_CHAIN of loss_kernels.h: the longest addition chain of the two sums"""
    tiles = planes * ((H + TILE_H - 1) // TILE_H) * ((W + TILE_W - 1) // TILE_W)
    return 2 + 8 + (tiles + 1023) // 1024 + 10


def window():
    g = [math.exp(-(i - R) ** 2 / (2.0 * 1.5 * 1.5)) for i in range(TAPS)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], np.float64).astype(F32)


def _taps(q, axis):
    """11-tap sum along ``axis`` (-1: H pass, -2: V pass), zero padding, index order from a zero accumulator"""
    w = window()
    n = q.shape[axis]
    pad = [(0, 0)] * q.ndim
    pad[axis] = (R, R)
    qp = np.pad(q, pad)
    acc = np.zeros_like(q)
    for k in range(TAPS):
        sl = [slice(None)] * q.ndim
        sl[axis] = slice(k, k + n)
        acc = acc + w[k] * qp[tuple(sl)]
    assert acc.dtype == F32
    return acc


def filt(q):
    return _taps(_taps(q, -1), -2)


def factors(lam, n):
    """the host's scalars: ka = f32((1 - lam) / N), kb = f32(lam / N), f32(1 / N), with lam the f32 the C ABI receives"""
    lam = float(F32(lam))
    return F32((1.0 - lam) / n), F32(lam / n), F32(1.0 / n)


def forward(x, y):
    """[planes,H,W] f32 -> dict(map, p0, p1, p2, absdiff), all [planes,H,W] f32"""
    x = np.ascontiguousarray(x, F32)
    y = np.ascontiguousarray(y, F32)
    two = F32(2)
    with np.errstate(all="ignore"):
        mu1, mu2 = filt(x), filt(y)
        exx, eyy, exy = filt(x * x), filt(y * y), filt(x * y)
        m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = exx - m11, eyy - m22, exy - m12
        A = (m11 + m22) + C1
        B = (s1 + s2) + C2
        C = two * m12 + C1
        D = two * s12 + C2
        AB = A * B
        m = (C * D) / AB
        mu1m = mu1 * m
        p0 = two * ((((mu2 * D) / AB - (mu2 * C) / AB) - mu1m / A) + mu1m / B)
        p1 = -(m / B)
        p2 = (two * C) / AB
        ad = np.abs(x - y)
    for a in (m, p0, p1, p2, ad):
        assert a.dtype == F32
    return dict(map=m, p0=p0, p1=p1, p2=p2, absdiff=ad)


def scalars64(fw, lam):
    """fp64 sums of the statement's f32 terms -> (loss, l1_mean, ssim_mean) and the sums of |terms| behind each"""
    n = fw["map"].size
    ka, kb, inv_n = (float(v) for v in factors(lam, n))
    s1 = float(fw["absdiff"].astype(np.float64).sum())
    sm = float(fw["map"].astype(np.float64).sum())
    am = float(np.abs(fw["map"]).astype(np.float64).sum())
    lam = float(F32(lam))
    value = (ka * s1 + lam - kb * sm, s1 * inv_n, sm * inv_n)
    absum = (ka * s1 + lam + kb * am, s1 * inv_n, am * inv_n)
    return value, absum


def backward(x, y, fw, lam, grad_loss=1.0):
    """dL/dx [planes,H,W] f32 from the statement's partials"""
    x = np.ascontiguousarray(x, F32)
    y = np.ascontiguousarray(y, F32)
    ka, kb, _ = factors(lam, x.size)
    gl = F32(grad_loss)
    g = gl * (-kb)
    l = gl * ka
    with np.errstate(all="ignore"):
        f0, f1, f2 = filt(g * fw["p0"]), filt(g * fw["p1"]), filt(g * fw["p2"])
        d = x - y
        sign = (d > 0).astype(F32) - (d < 0).astype(F32)
        dx = ((f0 + (F32(2) * x) * f1) + y * f2) + l * sign
    assert dx.dtype == F32
    return dx
