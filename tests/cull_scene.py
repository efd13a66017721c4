"""Synthetic DTU-style scans for the cull tests: cameras on a ring that look at the object's centre, written as the
``world_mat_i`` / ``scale_mat_i`` pairs of a cameras.npz, disc masks, and points in the normalised frame."""
import numpy as np

SCALE, CENTRE = 1.3, np.array([0.1, -0.2, 0.05])          # scale_mat: normalised frame -> world = SCALE * p + CENTRE


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world-to-camera rotation with +z towards the target, +x right, +y down"""
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def cameras(n, image_size, seed=0):
    """-> (dict of world_mat_i / scale_mat_i [4,4] f64, list of (K, R, C) they were built from).  The cameras stand 3.2 to 4
    world units from CENTRE and see a ball of radius 1 around it at about two thirds of the image height."""
    W, H = image_size
    rng = np.random.default_rng(seed)
    out, parts = {}, []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1) + 0.3
        C = CENTRE + np.array([np.cos(a), np.sin(a), 0.35 + 0.1 * i]) * (3.2 + 0.4 * i)
        R = look_at(C, CENTRE + rng.normal(0, 0.02, 3))
        f = 1.1 * H
        K = np.array([[f, 0.3, (W - 1) / 2 + 1.7], [0, f * 1.01, (H - 1) / 2 - 0.9], [0, 0, 1.0]])
        P = np.eye(4)
        P[:3, :3] = K @ R
        P[:3, 3] = -K @ R @ C
        P[:3] *= 1.7 + i                                     # a projection matrix is defined up to its scale
        S = np.eye(4)
        S[:3, :3] *= SCALE
        S[:3, 3] = CENTRE
        out[f"world_mat_{i}"], out[f"scale_mat_{i}"] = P, S
        parts.append((K, R, C))
    return out, parts


def disc_masks(n, mask_size, radius_share=0.3):
    """[n,H,W] u8: a disc (0 / 255) a little off the centre of every view"""
    W, H = mask_size
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(((x - W / 2 - 2 * i) ** 2 + (y - H / 2 + i) ** 2) <= (radius_share * H) ** 2).astype(np.uint8) * 255
                     for i in range(n)])


def points(V, seed=0, half=1.1):
    """[V,3] f32 in the normalised frame: uniform in a cube that reaches past the edges of every view"""
    return np.random.default_rng(seed).uniform(-half, half, (V, 3)).astype(np.float32)


def sphere_mesh(n_lat=24, n_lon=48, radius=0.8):
    """(vertices [V,3] f64, triangles [T,3] int32) of a latitude / longitude sphere in the normalised frame"""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, Pp = np.meshgrid(th, ph, indexing="ij")
    v = radius * np.stack([np.sin(T) * np.cos(Pp), np.sin(T) * np.sin(Pp), np.cos(T)], -1).reshape(-1, 3)
    v = np.concatenate([v, [[0, 0, radius], [0, 0, -radius]]])
    rows, top, bottom = n_lat - 1, len(v) - 2, len(v) - 1
    tris = []
    for r in range(rows - 1):
        for c in range(n_lon):
            a, b = r * n_lon + c, r * n_lon + (c + 1) % n_lon
            tris += [[a, a + n_lon, b + n_lon], [a, b + n_lon, b]]
    for c in range(n_lon):
        tris.append([top, c, (c + 1) % n_lon])
        tris.append([bottom, (rows - 1) * n_lon + (c + 1) % n_lon, (rows - 1) * n_lon + c])
    return v, np.asarray(tris, np.int32)
