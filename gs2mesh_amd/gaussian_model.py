"""Gaussian store of GS/scene/gaussian_model.py: the inference part the hot path touches, and the training half
(initialisation from a point cloud, Adam groups, densification and pruning with the optimiser surgery they need).

  * ``load_ply``  (gaussian_model.py:215-256; attribute order :177-189):
    reads ``point_cloud/iteration_N/point_cloud.ply`` without ``plyfile`` -- one ``vertex`` element of
    float32 properties ``x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3``;
    ``f_rest`` is channel-major on disk (j = c*15 + k-1) and coefficient-major in memory [P,15,3].
  * getters with the reference's activations (gaussian_model.py:95-115) for the operator-level API;
  * ``raw()``: the pre-activation tensors for the fused pipeline-level API (no ``torch.cat`` of
    dc/rest per call, no separate exp / normalize / sigmoid passes).
  * training half (gaussian_model.py:61-93, 120-175, 210-213, 258-407): ``create_from_pcd``, ``training_setup``,
    ``densify_and_prune`` and what they are built from, restated with every tensor on ``self.device``.
Importing this module does not need ``simple_knn`` (the reference imports it at module scope,
gaussian_model.py:20; here ``create_from_pcd`` imports the HIP ``distCUDA2`` when it runs) nor a GPU.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .sh_utils import RGB2SH


def read_gaussian_ply(path):
    """-> dict of float32 numpy arrays: xyz[P,3], f_dc[P,3], f_rest[P,R], opacity[P,1], scale[P,3], rot[P,4]."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n, props, in_vertex = None, None, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.strip().split()
            if not tok:
                continue
            if tok[0] == b"format":
                fmt = tok[1].decode()
            elif tok[0] == b"element":
                in_vertex = tok[1] == b"vertex"
                if in_vertex:
                    n = int(tok[2])
            elif tok[0] == b"property" and in_vertex:
                if tok[1] == b"list":
                    raise ValueError("list property in vertex element")
                props.append((tok[2].decode(), tok[1].decode()))
            elif tok[0] == b"end_header":
                break
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        ch = "<" if fmt == "binary_little_endian" else ">"
        tmap = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1",
                "int": "i4", "int32": "i4", "uint": "u4", "short": "i2", "ushort": "u2", "char": "i1"}
        dt = np.dtype([(name, ch + tmap[t]) for name, t in props])
        data = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
    col = lambda name: np.asarray(data[name], np.float32)
    names = [p[0] for p in props]
    srt = lambda pre: sorted([k for k in names if k.startswith(pre)], key=lambda x: int(x.split("_")[-1]))
    rest = srt("f_rest_")
    return dict(
        xyz=np.stack([col("x"), col("y"), col("z")], 1),
        f_dc=np.stack([col("f_dc_0"), col("f_dc_1"), col("f_dc_2")], 1),
        f_rest=np.stack([col(k) for k in rest], 1) if rest else np.zeros((n, 0), np.float32),
        opacity=col("opacity")[:, None],
        scale=np.stack([col(k) for k in srt("scale_")], 1),
        rot=np.stack([col(k) for k in srt("rot")], 1))


def write_gaussian_ply(path, xyz, features_dc, features_rest, opacity, scaling, rotation):
    """Inverse of ``read_gaussian_ply`` in the layout GaussianModel.save_ply writes
    (gaussian_model.py:191-208): float32, binary little endian, f_rest channel-major."""
    P = xyz.shape[0]
    f_dc = np.asarray(features_dc, np.float32).transpose(0, 2, 1).reshape(P, -1)
    f_rest = np.asarray(features_rest, np.float32).transpose(0, 2, 1).reshape(P, -1)
    cols = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(f_dc.shape[1])] + \
           [f"f_rest_{i}" for i in range(f_rest.shape[1])] + ["opacity"] + \
           [f"scale_{i}" for i in range(scaling.shape[1])] + [f"rot_{i}" for i in range(rotation.shape[1])]
    arr = np.concatenate([np.asarray(xyz, np.float32), np.zeros((P, 3), np.float32), f_dc, f_rest,
                          np.asarray(opacity, np.float32).reshape(P, 1), np.asarray(scaling, np.float32),
                          np.asarray(rotation, np.float32)], axis=1).astype("<f4")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\n")
        f.write(f"element vertex {P}\n".encode())
        for c in cols:
            f.write(f"property float {c}\n".encode())
        f.write(b"end_header\n")
        f.write(arr.tobytes())


def inverse_sigmoid(x):
    """utils/general_utils.py:18-19"""
    return torch.log(x / (1 - x))


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:28-62: step -> learning rate, log-linear from ``lr_init`` (step 0) to ``lr_final``
    (``max_steps``), times a sine ease-in from ``lr_delay_mult`` to 1 over the first ``lr_delay_steps`` steps."""
    def rate(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        t = np.clip(step / max_steps, 0, 1)
        return delay * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)

    return rate


def build_rotation(r):
    """utils/general_utils.py:78-100: [P,4] quaternions (r, x, y, z), not necessarily unit -> [P,3,3]"""
    q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


# optimiser group name -> attribute, in the order of the reference's param_groups (gaussian_model.py:154-161)
_GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
           ("scaling", "_scaling"), ("rotation", "_rotation"))


class GaussianModel:
    def __init__(self, sh_degree: int, device="cuda"):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self.device = device
        e = torch.empty(0)
        self._xyz = self._features_dc = self._features_rest = self._scaling = self._rotation = self._opacity = e
        self.max_radii2D = self.xyz_gradient_accum = self.denom = e
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0

    # ---- GS/scene/gaussian_model.py:95-115 ---------------------------------------------------
    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier=1.0):
        """GS/scene/gaussian_model.py:117-118 -> build_covariance_from_scaling_rotation (:27-31): Sigma = L L^T with
        L = R(q / |q|) diag(modifier * exp(scaling)), returned as the 6 upper-triangle entries
        [xx, xy, xz, yy, yz, zz] (general_utils.strip_lowerdiag) -- the layout the rasteriser's cov3D_precomp takes."""
        q = torch.nn.functional.normalize(self._rotation)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
        L = R * (scaling_modifier * self.get_scaling).unsqueeze(1)      # R @ diag(s)
        S = L @ L.transpose(1, 2)
        return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)

    def load_ply(self, path):
        d = read_gaussian_ply(path)
        P = d["xyz"].shape[0]
        n_rest = 3 * (self.max_sh_degree + 1) ** 2 - 3
        assert d["f_rest"].shape[1] == n_rest, (d["f_rest"].shape, n_rest)
        f_rest = d["f_rest"].reshape(P, 3, (self.max_sh_degree + 1) ** 2 - 1).transpose(0, 2, 1)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.device)
        self._xyz = t(d["xyz"])
        self._features_dc = t(d["f_dc"][:, None, :])
        self._features_rest = t(f_rest)
        self._opacity = t(d["opacity"])
        self._scaling = t(d["scale"])
        self._rotation = t(d["rot"])
        self.active_sh_degree = self.max_sh_degree

    def load_arrays(self, xyz, features_dc, features_rest, scaling, rotation, opacity):
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.device)
        self._xyz, self._features_dc, self._features_rest = t(xyz), t(features_dc), t(features_rest)
        self._scaling, self._rotation, self._opacity = t(scaling), t(rotation), t(opacity)
        self.active_sh_degree = self.max_sh_degree

    def save_ply(self, path):
        c = lambda x: x.detach().cpu().numpy()
        write_gaussian_ply(path, c(self._xyz), c(self._features_dc), c(self._features_rest), c(self._opacity),
                           c(self._scaling), c(self._rotation))

    def raw(self):
        """Pre-activation tensors for ``Rasterizer.render_views`` (activations fused in-kernel)."""
        return dict(xyz=self._xyz, scaling=self._scaling, rotation=self._rotation, opacity=self._opacity,
                    features_dc=self._features_dc, features_rest=self._features_rest, raw=True,
                    sh_degree=self.active_sh_degree)

    # ---- training half ------------------------------------------------------------------------------------------------
    def capture(self):
        """gaussian_model.py:61-75"""
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        """gaussian_model.py:77-93"""
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
         self._opacity, self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        self.training_setup(training_args)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def create_from_pcd(self, pcd, spatial_lr_scale: float):
        """gaussian_model.py:124-147: centres = the points, DC colour = RGB2SH(colours), rest SH 0, isotropic scale = the
        root of the mean squared distance to the three nearest points (``distCUDA2``, floor 1e-7), identity rotation,
        opacity 0.1.  ``pcd``: ``graphics.BasicPointCloud``."""
        from .simple_knn._C import distCUDA2        # the HIP library: needed when a cloud is initialised, not at import
        self.spatial_lr_scale = spatial_lr_scale
        dev = self.device
        xyz = torch.tensor(np.asarray(pcd.points)).float().to(dev)
        P = xyz.shape[0]
        n_coef = (self.max_sh_degree + 1) ** 2
        f_dc = RGB2SH(torch.tensor(np.asarray(pcd.colors)).float().to(dev)).reshape(P, 1, 3)
        f_rest = torch.zeros((P, n_coef - 1, 3), dtype=torch.float32, device=dev)
        dist2 = torch.clamp_min(distCUDA2(xyz), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((P, 4), device=dev)
        rots[:, 0] = 1
        opacities = inverse_sigmoid(0.1 * torch.ones((P, 1), dtype=torch.float32, device=dev))
        self._xyz = nn.Parameter(xyz.requires_grad_(True))
        self._features_dc = nn.Parameter(f_dc.contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(f_rest.requires_grad_(True))
        self._scaling = nn.Parameter(scales.requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(opacities.requires_grad_(True))
        self.max_radii2D = torch.zeros(P, device=dev)

    def training_setup(self, training_args):
        """gaussian_model.py:149-167.  Plain tensors (``load_ply`` / ``load_arrays``) become Parameters first, so a loaded
        splat can be fine-tuned."""
        for _, attr in _GROUPS:
            t = getattr(self, attr)
            if not isinstance(t, nn.Parameter):
                setattr(self, attr, nn.Parameter(t.detach().to(self.device).contiguous().requires_grad_(True)))
        P = self._xyz.shape[0]
        self.percent_dense = training_args.percent_dense
        self.xyz_gradient_accum = torch.zeros((P, 1), device=self.device)
        self.denom = torch.zeros((P, 1), device=self.device)
        if self.max_radii2D.shape[0] != P:
            self.max_radii2D = torch.zeros(P, device=self.device)
        a = training_args
        lr = {"xyz": a.position_lr_init * self.spatial_lr_scale, "f_dc": a.feature_lr, "f_rest": a.feature_lr / 20.0,
              "opacity": a.opacity_lr, "scaling": a.scaling_lr, "rotation": a.rotation_lr}
        groups = [{"params": [getattr(self, attr)], "lr": lr[name], "name": name} for name, attr in _GROUPS]
        kind = getattr(a, "optimizer_type", "default")
        if kind == "default":
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        elif kind in ("fused", "sparse_adam"):
            from .optim import FusedAdam
            self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        else:
            raise ValueError(f"optimizer_type must be 'default', 'fused' or 'sparse_adam', got {kind!r}")
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=a.position_lr_init * self.spatial_lr_scale,
                                                    lr_final=a.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=a.position_lr_delay_mult,
                                                    max_steps=a.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        """gaussian_model.py:169-175: only the positions are scheduled"""
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = lr = self.xyz_scheduler_args(iteration)
                return lr

    def reset_opacity(self):
        """gaussian_model.py:210-213"""
        op = self.get_opacity
        new = inverse_sigmoid(torch.min(op, torch.ones_like(op) * 0.01))
        self._opacity = self.replace_tensor_to_optimizer(new, "opacity")["opacity"]

    # -- optimiser surgery (gaussian_model.py:258-327): every group holds one Parameter; when its rows change, the Parameter
    # -- is replaced and the Adam moments follow it (zeros for new rows) ---------------------------------------------------
    def _swap(self, group, new_tensor, moments):
        """put ``new_tensor`` in ``group``; ``moments``: old state dict -> (exp_avg, exp_avg_sq) of the new Parameter"""
        old = group["params"][0]
        state = self.optimizer.state.get(old, None)
        if state is not None:
            if "exp_avg" in state:
                state["exp_avg"], state["exp_avg_sq"] = moments(state)
            del self.optimizer.state[old]
        group["params"][0] = nn.Parameter(new_tensor.detach().requires_grad_(True))
        if state is not None:
            self.optimizer.state[group["params"][0]] = state
        return group["params"][0]

    def _assign(self, tensors):
        for name, attr in _GROUPS:
            if name in tensors:
                setattr(self, attr, tensors[name])

    def replace_tensor_to_optimizer(self, tensor, name):
        out = {}
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                out[name] = self._swap(group, tensor, lambda st: (torch.zeros_like(tensor), torch.zeros_like(tensor)))
        return out

    def _prune_optimizer(self, mask):
        out = {}
        for group in self.optimizer.param_groups:
            out[group["name"]] = self._swap(group, group["params"][0].detach()[mask],
                                            lambda st: (st["exp_avg"][mask], st["exp_avg_sq"][mask]))
        return out

    def prune_points(self, mask):
        """gaussian_model.py:291-305: drop the rows where ``mask`` is set"""
        keep = ~mask
        self._assign(self._prune_optimizer(keep))
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
        self.denom = self.denom[keep]
        self.max_radii2D = self.max_radii2D[keep]

    def cat_tensors_to_optimizer(self, tensors_dict):
        out = {}
        for group in self.optimizer.param_groups:
            assert len(group["params"]) == 1
            ext = tensors_dict[group["name"]].detach()
            grow = lambda st, ext=ext: (torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0),
                                        torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0))
            out[group["name"]] = self._swap(group, torch.cat((group["params"][0].detach(), ext), dim=0), grow)
        return out

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling, new_rotation):
        """gaussian_model.py:329-347: append rows; the densification statistics start again"""
        self._assign(self.cat_tensors_to_optimizer({"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest,
                                                    "opacity": new_opacities, "scaling": new_scaling,
                                                    "rotation": new_rotation}))
        P = self._xyz.shape[0]
        self.xyz_gradient_accum = torch.zeros((P, 1), device=self.device)
        self.denom = torch.zeros((P, 1), device=self.device)
        self.max_radii2D = torch.zeros(P, device=self.device)

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2):
        """gaussian_model.py:349-372: large Gaussians with a high positional gradient are replaced by N samples of
        themselves, scale / (0.8 N).  ``grads`` may be shorter than the model (rows cloned just before): padded with 0."""
        P = self._xyz.shape[0]
        padded = torch.zeros(P, device=self.device)
        padded[:grads.shape[0]] = grads.squeeze()
        sel = torch.logical_and(padded >= grad_threshold,
                                torch.max(self.get_scaling, dim=1).values > self.percent_dense * scene_extent)
        stds = self.get_scaling[sel].repeat(N, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=self.device), std=stds)
        rots = build_rotation(self._rotation[sel]).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self._xyz[sel].repeat(N, 1)
        new_scaling = torch.log(self.get_scaling[sel].repeat(N, 1) / (0.8 * N))
        self.densification_postfix(new_xyz, self._features_dc[sel].repeat(N, 1, 1), self._features_rest[sel].repeat(N, 1, 1),
                                   self._opacity[sel].repeat(N, 1), new_scaling, self._rotation[sel].repeat(N, 1))
        k = int(sel.sum())
        self.prune_points(torch.cat((sel, torch.zeros(N * k, device=self.device, dtype=torch.bool))))
        return k

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        """gaussian_model.py:374-387: small Gaussians with a high positional gradient are duplicated"""
        sel = torch.logical_and(torch.norm(grads, dim=-1) >= grad_threshold,
                                torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        new_xyz = self._xyz[sel]
        self.densification_postfix(new_xyz, self._features_dc[sel], self._features_rest[sel], self._opacity[sel],
                                   self._scaling[sel], self._rotation[sel])
        return new_xyz.shape[0]

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        """gaussian_model.py:389-403.  -> {"cloned", "split", "pruned"}: the rows each step touched (the reference returns
        nothing; the counts are already on the host)."""
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        cloned = self.densify_and_clone(grads, max_grad, extent)
        split = self.densify_and_split(grads, max_grad, extent)
        before = self._xyz.shape[0]
        prune = (self.get_opacity < min_opacity).squeeze(-1)
        if max_screen_size:
            big_vs = self.max_radii2D > max_screen_size
            big_ws = self.get_scaling.max(dim=1).values > 0.1 * extent
            prune = torch.logical_or(torch.logical_or(prune, big_vs), big_ws)
        self.prune_points(prune)
        return {"cloned": cloned, "split": split, "pruned": before - self._xyz.shape[0]}

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        """gaussian_model.py:405-407"""
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1,
                                                             keepdim=True)
        self.denom[update_filter] += 1

    def update_densification_stats(self, viewspace_point_tensor, radii):
        """``max_radii2D[visible] = max(...)`` of the loop and ``add_densification_stats`` as one kernel
        (``gs2m_densify_stats``) over the rows with ``radii > 0``; no mask is materialised and the host does not wait."""
        from .optim import densify_stats
        grad = viewspace_point_tensor.grad
        densify_stats(radii, grad if grad.is_contiguous() else grad.contiguous(), self.max_radii2D, self.xyz_gradient_accum,
                      self.denom)
