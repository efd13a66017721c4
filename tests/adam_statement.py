"""Plain numpy statement of gs2m_adam_step and gs2m_densify_stats (include/gs2mesh_amd.h,
gs2mesh_amd/csrc/optim_kernels.h): every operation is one float32 operation, in the order the header fixes.

  scalars   in double, cast to f32 last: ss = lr / (1 - beta1^t), bs = sqrt(1 - beta2^t), omb1 = 1 - beta1, b2 = beta2,
            omb2 = 1 - beta2, e = eps;  beta^t = pow(beta, float(t))
  step      m' = m + omb1 * (g - m);  v' = b2 * v + (omb2 * g) * g;  p' = p - ss * (m' / (sqrt(v') / bs + e))
  sparse    rows with row_visible <= 0 keep p, m, v bit for bit, whatever their gradient holds
  stats     where radii > 0: max_radii2D = r > max_radii2D ? r : max_radii2D, grad_accum += sqrt(gx * gx + gy * gy), denom += 1
"""
import math

import numpy as np

F32 = np.float32
WG_ELEMS = 1024                         # ADAM_WG_ELEMS: a workgroup's elements; 4 per lane


def scalars(lr, betas, eps, t):
    b1, b2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    return dict(ss=F32(float(lr) / bc1), bs=F32(math.sqrt(bc2)), omb1=F32(1.0 - b1), b2=F32(b2), omb2=F32(1.0 - b2), e=F32(eps))


def adam(p, g, m, v, lr, betas, eps, t, row_visible=None):
    """-> (p', m', v'), new float32 arrays of the inputs' shape.  ``row_visible``: None or one int per leading row."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    c = scalars(lr, betas, eps, t)
    with np.errstate(all="ignore"):
        m2 = m + c["omb1"] * (g - m)
        v2 = c["b2"] * v + (c["omb2"] * g) * g
        p2 = p - c["ss"] * (m2 / (np.sqrt(v2) / c["bs"] + c["e"]))
    assert p2.dtype == F32 and m2.dtype == F32 and v2.dtype == F32
    if row_visible is not None:
        seen = (np.asarray(row_visible) > 0).reshape((-1,) + (1,) * (p.ndim - 1))
        p2, m2, v2 = np.where(seen, p2, p), np.where(seen, m2, m), np.where(seen, v2, v)
    return p2, m2, v2


def adam64(p, g, m, v, lr, betas, eps, t):
    """Adam in double on the given values (the yardstick of the statement, never of the kernel): torch.optim.Adam's formulas."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    p2 = p - (lr / (1.0 - b1 ** t)) * m2 / (np.sqrt(v2) / math.sqrt(1.0 - b2 ** t) + eps)
    return p2, m2, v2


def densify_stats(radii, viewspace_grad, max_radii2D, grad_accum, denom):
    """-> (max_radii2D', grad_accum', denom'), new float32 arrays"""
    radii = np.asarray(radii)
    g = np.asarray(viewspace_grad, F32)
    mr, acc, den = (np.asarray(a, F32) for a in (max_radii2D, grad_accum, denom))
    seen = (radii > 0).reshape(mr.shape)
    r = radii.astype(F32).reshape(mr.shape)
    with np.errstate(all="ignore"):
        n = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        mr2 = np.where(seen, np.where(r > mr, r, mr), mr)
        acc2 = np.where(seen.reshape(acc.shape), acc + n.reshape(acc.shape), acc)
        den2 = np.where(seen.reshape(den.shape), den + F32(1.0), den)
    assert n.dtype == F32 and acc2.dtype == F32 and den2.dtype == F32 and mr2.dtype == F32
    return mr2, acc2, den2
