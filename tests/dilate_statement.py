"""The statement gs2m_mask_dilate_disk is tested against: the routine the reference's
``skimage.morphology.binary_dilation(mask, disk(24))`` (evaluation/DTU/eval_code/evaluate_single_scene.py:80) resolves to,
``scipy.ndimage.binary_dilation`` with skimage's ``disk`` footprint (X^2 + Y^2 <= r^2) and the default 0 border."""
import numpy as np
from scipy import ndimage


def disk(r):
    """skimage.morphology.disk(r): uint8 [2r+1, 2r+1], 1 where X^2 + Y^2 <= r^2"""
    L = np.arange(-r, r + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= r ** 2, dtype=np.uint8)


def dilate(mask, r):
    """[H,W] anything -> [H,W] bool"""
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=disk(r))


def pack(m):
    """[..., H, W] bool -> [..., H, nw] uint64: bit x & 63 of word x >> 6 is pixel x, the bits at x >= W are 0"""
    m = np.asarray(m, bool)
    W = m.shape[-1]
    nw = (W + 63) // 64
    padded = np.zeros(m.shape[:-1] + (nw * 64,), bool)
    padded[..., :W] = m
    bits = np.packbits(padded.reshape(m.shape[:-1] + (nw, 64)), axis=-1, bitorder="little")      # 8 bytes a word, byte 0 = bits 0-7
    return np.ascontiguousarray(bits).view("<u8").reshape(m.shape[:-1] + (nw,))
