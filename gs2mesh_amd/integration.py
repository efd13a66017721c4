"""Open3D-shaped front-end of the HIP TSDF integrator (the subset gs2mesh_utils/tsdf_utils.py uses).

    volume = ScalableTSDFVolume(voxel_length, sdf_trunc, color_type=TSDFVolumeColorType.RGB8)
    rgbd   = RGBDImage.create_from_color_and_depth(Image(rgb), Image(depth), depth_scale=..,
                                                   depth_trunc=.., convert_rgb_to_intensity=False)
    volume.integrate(rgbd, PinholeCameraIntrinsic(w, h, fx, fy, cx, cy), extrinsic_world_to_cam)

mirrors ``o3d.pipelines.integration.ScalableTSDFVolume`` / ``o3d.geometry.RGBDImage`` /
``o3d.camera.PinholeCameraIntrinsic`` as called at tsdf_utils.py:53-56,88-93,106-107 (same names,
argument meaning and error text).  Images may be numpy arrays (uploaded) or torch tensors already
on the device (the in-memory render -> fuse hand-off).  The depth conversion
(depth/scale, >= trunc -> 0) is recorded lazily and fused into the integration kernels.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import _is_torch, _ptr, _stream_of

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class TSDFVolumeColorType(enum.IntEnum):
    NoColor = 0
    RGB8 = 1
    Gray32 = 2


class PinholeCameraIntrinsic:
    def __init__(self, width, height, fx, fy, cx, cy):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)

    @property
    def intrinsic_matrix(self):
        return np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1.0]])


class Image:
    """o3d.geometry.Image stand-in: wraps an array, no copy."""

    def __init__(self, data):
        self.data = data

    @property
    def shape(self):
        return tuple(self.data.shape)


class RGBDImage:
    def __init__(self, color, depth, depth_scale=1.0, depth_trunc=float("inf")):
        self.color, self.depth = color, depth
        self.depth_scale, self.depth_trunc = float(depth_scale), float(depth_trunc)

    @staticmethod
    def create_from_color_and_depth(color, depth, depth_scale=1000.0, depth_trunc=3.0,
                                    convert_rgb_to_intensity=True):
        if convert_rgb_to_intensity:
            raise NotImplementedError("convert_rgb_to_intensity=True is not on the GS2Mesh path "
                                      "(tsdf_utils.py:93 passes False)")
        c = color.data if isinstance(color, Image) else color
        d = depth.data if isinstance(depth, Image) else depth
        if tuple(c.shape[:2]) != tuple(d.shape[:2]):
            raise RuntimeError("[CreateFromColorAndDepth] Unsupported image format.")
        return RGBDImage(c, d, depth_scale, depth_trunc)


class ScalableTSDFVolume:
    """HIP block-sparse TSDF volume.  ``max_blocks`` sizes the 16^3-voxel block pool
    (80 KiB per block; default 32768 blocks = 2.7 GB = a dense 512^3 volume)."""

    def __init__(self, voxel_length, sdf_trunc, color_type=TSDFVolumeColorType.RGB8, volume_unit_resolution=16,
                 depth_sampling_stride=4, max_blocks=32768, device=0, lib=None):
        self._lib = lib or _lib.get()
        if int(color_type) not in (0, 1):
            raise NotImplementedError("only NoColor / RGB8 volumes (tsdf_utils.py:56 uses RGB8)")
        self.voxel_length = float(voxel_length)
        self.sdf_trunc = float(sdf_trunc)
        self.color_type = TSDFVolumeColorType(int(color_type))
        self.max_blocks = int(max_blocks)
        self.device = device
        h = C.c_void_p()
        _lib.check(self._lib.gs2m_tsdf_create(C.byref(h), self.voxel_length, self.sdf_trunc, int(color_type),
                                              int(volume_unit_resolution), int(depth_sampling_stride),
                                              self.max_blocks, int(device)), self._lib)
        self._h = h
        self._keep = []  # uploaded frames stay alive until the next synchronising call
        # frames this volume's state carries = an upper bound of every voxel weight (the packed exchange form needs it):
        # upper bound of every voxel weight, in three parts (gs2mesh_amd.parallel sums them correctly across ranks):
        # `frames_base` = inherited from a REDUCTION (a reduce-scatter leaves the ranks with disjoint parts of one reduced
        # volume: across ranks these bounds do not add up, their maximum holds), `frames_injected` = state the caller put
        # in with unpack(..., frames=F) (several ranks may inject into the SAME blocks, e.g. one checkpoint loaded everywhere:
        # these add up), `frames_local` = frames integrated here since (add up)
        self.frames_base = 0
        self.frames_injected = 0
        self.frames_local = 0
        self.replicated = False      # the state is the all-reduced volume (every rank holds it: summing it again would count it R times)
        self.has_halo = False        # holds neighbour-only copies of other ranks' blocks (exchange_halo): their keys read as the sentinel
        # window of block indices of the block-map key exchange (gs2mesh_amd.parallel): (lo[3], dim[3]); the default covers a
        # 1024^3-voxel volume around the origin (64^3 blocks = a 256 KiB byte map).  A block outside it sends the exchange through
        # the gather path (same result); `set_exchange_window` for scenes elsewhere.
        self.exchange_window = ((-32, -32, -32), (64, 64, 64))
        self._xbuf = {}              # persistent, grow-only exchange buffers (gs2mesh_amd.parallel)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gs2m_tsdf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=None):
        _lib.check(self._lib.gs2m_tsdf_reset(self._h, stream or C.c_void_p(0)), self._lib)
        self._reset_bookkeeping()

    def _reset_bookkeeping(self):
        self.frames_base = self.frames_local = self.frames_injected = 0
        self.replicated = False
        self.has_halo = False

    @property
    def frames_integrated(self):
        return self.frames_base + self.frames_injected + self.frames_local

    def exchange_buffer(self, name, shape, dtype, device):
        """A persistent, grow-only device buffer owned by the volume (the multi-GPU reduction re-uses its pack / receive
        buffers across calls instead of allocating GBs per reduction); returns a view of ``shape``."""
        n = 1
        for d in shape:
            n *= int(d)
        cur = self._xbuf.get(name)
        if cur is None or cur.dtype != dtype or cur.numel() < n or cur.device != torch.device(device):
            self._xbuf[name] = cur = torch.empty(max(n + n // 8, 1), dtype=dtype, device=device)
        return cur[:n].view(*shape)

    # ---------------------------------------------------------------------------------------
    def _to_dev(self, a, dtype):
        """host array / tensor -> contiguous device tensor of ``dtype`` (``_lib.MEMORY.upload``)."""
        if a is None:
            return None
        return _lib.MEMORY.upload(a, dtype, self.device)

    def _frame_to_dev(self, image, mask, intrinsic):
        """``(image, mask)`` -> the device tensors ``(depth, color, mask)`` the kernels read (``color`` only for a volume
        with colour, ``mask`` only when given), checked against ``intrinsic`` as Open3D checks them."""
        f32 = torch.float32 if torch is not None else None
        u8 = torch.uint8 if torch is not None else None
        has_color = self.color_type == TSDFVolumeColorType.RGB8
        depth = self._to_dev(image.depth, f32)
        color = self._to_dev(image.color, u8) if has_color else None
        msk = self._to_dev(mask, u8) if mask is not None else None
        H, W = int(depth.shape[0]), int(depth.shape[1])
        bad = W != intrinsic.width or H != intrinsic.height or depth.ndim != 2
        if has_color:
            bad = bad or color is None or color.ndim != 3 or tuple(color.shape) != (H, W, 3)
        if bad:
            raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
        return depth, color, msk

    def integrate(self, image: RGBDImage, intrinsic: PinholeCameraIntrinsic, extrinsic, mask=None, min_depth=0.0,
                  stream=None):
        """``volume.integrate(rgbd, intrinsic, extrinsic_world_to_camera)``.  Extras (fused
        TSDF.run preprocessing, tsdf_utils.py:68-83): ``mask`` [H,W] (depth *= mask != 0) and
        ``min_depth`` (depth < min_depth -> 0), both applied before the scale/trunc conversion."""
        depth, color, msk = self._frame_to_dev(image, mask, intrinsic)
        # buffers WE created (uploads / dtype conversions) must outlive the asynchronous kernels;
        # caller-owned device tensors are the caller's to keep alive until it synchronises
        ours = [t for t, src in ((depth, image.depth), (color, image.color), (msk, mask))
                if t is not None and t is not src]
        E = np.ascontiguousarray(np.asarray(extrinsic, np.float64).reshape(4, 4))
        st = _stream_of(depth, stream)
        _lib.check(self._lib.gs2m_tsdf_integrate(
            self._h, _ptr(depth), _ptr(color), _ptr(msk), intrinsic.width, intrinsic.height, intrinsic.fx, intrinsic.fy,
            intrinsic.cx, intrinsic.cy, E.ctypes.data_as(C.POINTER(C.c_double)), float(image.depth_scale),
            float(image.depth_trunc), float(min_depth), st), self._lib)
        self.frames_local += 1
        if ours:
            self._keep.append(ours)
            if len(self._keep) > 64:
                self.status(stream)

    def integrate_batch(self, images, intrinsic: PinholeCameraIntrinsic, extrinsics, masks=None, min_depth=0.0, stream=None):
        """``gs2m_tsdf_integrate_batch``: the frames ``images`` (list of RGBDImage sharing depth_scale / depth_trunc) under
        ``extrinsics`` (list of 4x4 world -> camera) in one voxel-stationary sweep; bit-identical to calling
        ``integrate`` on them in list order."""
        n = len(images)
        if n == 0:
            return
        if len(extrinsics) != n or (masks is not None and len(masks) != n):
            raise ValueError("integrate_batch: images / extrinsics / masks must have the same length")
        has_color = self.color_type == TSDFVolumeColorType.RGB8
        keep, dp, cp, mp = [], (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, im in enumerate(images):
            if (im.depth_scale, im.depth_trunc) != (images[0].depth_scale, images[0].depth_trunc):
                raise ValueError("integrate_batch: the frames of a batch share one depth_scale / depth_trunc")
            d, c, m = self._frame_to_dev(im, masks[i] if masks is not None else None, intrinsic)
            keep += [d, c, m]
            dp[i], cp[i], mp[i] = _ptr(d), _ptr(c), _ptr(m)
        E = np.ascontiguousarray(np.stack([np.asarray(e, np.float64).reshape(4, 4) for e in extrinsics]))
        st = _stream_of(keep[0], stream)
        _lib.check(self._lib.gs2m_tsdf_integrate_batch(
            self._h, n, dp, cp if has_color else None, mp if masks is not None else None, intrinsic.width, intrinsic.height,
            intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy, E.ctypes.data_as(C.POINTER(C.c_double)),
            float(images[0].depth_scale), float(images[0].depth_trunc), float(min_depth), st), self._lib)
        self.frames_local += n
        self._keep.append(keep)      # the frames stay alive until the next synchronising call
        if len(self._keep) > 64:
            self.status(stream)

    def status(self, stream=None, raise_on_overflow=True):
        """Synchronises -> (n_blocks, block_updates, overflow_flags); raises on overflow (unless told not to: the
        multi-GPU reduction first agrees on the flag across ranks, then raises everywhere together)."""
        nb, bu, ov = C.c_int64(0), C.c_int64(0), C.c_int(0)
        _lib.check(self._lib.gs2m_tsdf_status(self._h, stream or C.c_void_p(0), C.byref(nb), C.byref(bu),
                                              C.byref(ov)), self._lib)
        self._keep.clear()
        if ov.value and raise_on_overflow:
            what = [n for b, n in ((1, "block pool exhausted (raise max_blocks)"), (2, "hash table full"),
                                   (4, "block index out of the +-2^20 range"),
                                   (8, "a voxel did not fit the packed exchange form (weight > 1023: use payload='f32')")) if ov.value & b]
            raise RuntimeError("TSDF volume overflow: " + ", ".join(what))
        return int(nb.value), int(bu.value), int(ov.value)

    def set_stage_timing(self, enable=True):
        _lib.check(self._lib.gs2m_tsdf_set_stage_timing(self._h, int(bool(enable))), self._lib)

    def stage_times(self, stream=None):
        ms = (C.c_double * 2)()
        cnt = (C.c_int64 * 2)()
        _lib.check(self._lib.gs2m_tsdf_stage_times(self._h, stream or C.c_void_p(0), ms, cnt), self._lib)
        return {name: (ms[i], cnt[i]) for i, name in enumerate(_lib.TSDF_STAGES)}

    @property
    def num_blocks(self):
        return self.status()[0]

    @property
    def voxel_updates(self):
        return self.status()[1] * 4096

    def download(self):
        """-> keys[n,3] i32, tsdf[n,4096] f32, weight[n,4096] f32, rgb_sum[n,4096,3] u32 (host numpy;
        voxel index x*256 + y*16 + z as Open3D's IndexOf).  Mean colour = rgb_sum / weight."""
        n = self.status()[0]
        keys = np.zeros((n, 3), np.int32)
        tsdf = np.zeros((n, 4096), np.float32)
        weight = np.zeros((n, 4096), np.float32)
        rgb = np.zeros((n, 4096, 3), np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        _lib.check(self._lib.gs2m_tsdf_download(self._h, C.c_void_p(0), n, vp(keys), vp(tsdf), vp(weight), vp(rgb)),
                   self._lib)
        return keys, tsdf, weight, rgb

    def extract_triangle_mesh(self, stream=None):
        """``volume.extract_triangle_mesh()`` (tsdf_utils.py:108): marching cubes AND the welding of its vertices on the GPU
        (``gs2m_tsdf_extract_mesh``: Open3D's edge -> vertex identity, first-appearance order); the indexed mesh is what crosses
        PCIe (vertices, colours, cut edges, triangle indices), and a device copy of the triangle indices stays attached for
        ``cluster_connected_triangles`` -> ``gs2mesh_amd.mesh.TriangleMesh``."""
        from .mesh import TriangleMesh
        # torch's current stream unless the caller names one: the device buffers below are zero-filled by torch on it, and the
        # integration work the caller queued there must be ordered before the extraction (not the NULL stream)
        st = C.c_void_p(int(stream)) if stream is not None else _lib.MEMORY.current_stream(self.device)
        nv, nt = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.gs2m_tsdf_extract_mesh(self._h, st, C.byref(nv), C.byref(nt)), self._lib)
        nv, nt = int(nv.value), int(nt.value)
        self.status(st)
        if nt == 0:
            return TriangleMesh()
        verts, cols = np.empty((nv, 3), np.float64), np.empty((nv, 3), np.float64)
        eidx, tri = np.empty((nv, 4), np.int32), np.empty((nt, 3), np.int32)
        hp = lambda a: C.c_void_p(a.ctypes.data)      # gs2m_tsdf_mesh_copy takes host or device destinations
        _lib.check(self._lib.gs2m_tsdf_mesh_copy(self._h, st, hp(verts), hp(cols), hp(eidx), hp(tri)), self._lib)
        tri_dev = _lib.MEMORY.zeros((nt, 3), np.int32, self.device)
        _lib.check(self._lib.gs2m_tsdf_mesh_copy(self._h, st, None, None, None, _ptr(tri_dev)), self._lib)
        m = TriangleMesh(verts, tri, cols if self.color_type == TSDFVolumeColorType.RGB8 else None)
        m.edge_index = eidx                      # [n_vertices, 4]: Open3D's vertex keys
        self.status(st)      # the device copy has landed (the clustering may be queued on another stream later)
        m.attach_device_triangles(tri_dev, self._lib, self.device)
        return m

    # -- multi-GPU exchange (gs2mesh_amd.parallel) -------------------------------------------
    def exchange_device(self):
        """where the exchange buffers of this volume live: the GPU, or the host for the emulator build (CPU tests)"""
        return _lib.MEMORY.buffer_device(self.device)

    def set_exchange_window(self, lo, dim):
        """Window of BLOCK indices (units of 16 voxels) the multi-GPU key exchange covers with its block map; every rank must set
        the same one."""
        lo, dim = tuple(int(x) for x in lo), tuple(int(x) for x in dim)
        if len(lo) != 3 or len(dim) != 3 or min(dim) <= 0 or dim[0] * dim[1] * dim[2] > (1 << 30):
            raise ValueError(f"bad exchange window {lo} {dim}")
        self.exchange_window = (lo, dim)

    def map_bytes(self, world):
        dim = (C.c_int32 * 3)(*self.exchange_window[1])
        return int(self._lib.gs2m_tsdf_map_bytes(dim, int(world)))

    def block_map(self, cells, rank, world, flags, stream=None):
        """``gs2m_tsdf_block_map``: this rank's blocks + header into ``cells`` (device uint8 [map_bytes(world)]); async."""
        lo = (C.c_int32 * 3)(*self.exchange_window[0])
        dim = (C.c_int32 * 3)(*self.exchange_window[1])
        _lib.check(self._lib.gs2m_tsdf_block_map(self._h, lo, dim, int(rank), int(world), int(self.frames_local + self.frames_injected),
                                                 int(self.frames_base), int(flags), _ptr(cells), _stream_of(cells, stream)),
                   self._lib)

    def map_keys(self, cells, world, keys_out, stream=None):
        """``gs2m_tsdf_map_keys`` on the reduced buffer: canonical keys into ``keys_out`` [max,3] + the header bytes (numpy
        uint8 [32 + 8 * world]).  Synchronises (the one host read of the key exchange)."""
        lo = (C.c_int32 * 3)(*self.exchange_window[0])
        dim = (C.c_int32 * 3)(*self.exchange_window[1])
        hdr = (C.c_uint8 * (_lib.TSDF_MAP_HEADER_BYTES + 8 * int(world)))()
        _lib.check(self._lib.gs2m_tsdf_map_keys(self._h, lo, dim, int(world), _ptr(cells), _ptr(keys_out), int(keys_out.shape[0]),
                                                hdr, _stream_of(cells, stream)), self._lib)
        return np.frombuffer(hdr, dtype=np.uint8).copy()

    def block_keys(self, like=None, stream=None, raise_on_overflow=True, out=None, n=None):
        """Keys of the allocated blocks, slot order (halo copies: sentinel key).  ``out`` / ``n``: write the first n rows of a
        caller buffer (n from a status() the caller already paid for: no synchronisation here)."""
        if out is not None:
            _lib.check(self._lib.gs2m_tsdf_block_keys(self._h, int(n), _ptr(out), _stream_of(out, stream)), self._lib)
            return out[: int(n)]
        n = min(self.status(stream, raise_on_overflow)[0], self.max_blocks)
        keys = _lib.MEMORY.zeros((n, 3), np.int32, self.device)
        _lib.check(self._lib.gs2m_tsdf_block_keys(self._h, n, _ptr(keys), _stream_of(keys, stream)), self._lib)
        return keys

    def pack(self, keys, form, buf_f32, buf_i64=None, stream=None):
        """``gs2m_tsdf_pack``: accumulators of the blocks ``keys`` [n,3] in exchange form ``form`` (_lib.XFORM_*)."""
        n = int(keys.shape[0])
        _lib.check(self._lib.gs2m_tsdf_pack(self._h, _ptr(keys), n, int(form), _ptr(buf_f32), _ptr(buf_i64),
                                            _stream_of(keys, stream)), self._lib)

    def unpack(self, keys, form, buf_f32, buf_i64=None, halo=False, stream=None, frames=None):
        """``gs2m_tsdf_unpack``: replace the state of the blocks ``keys`` from buffers in exchange form ``form``.
        ``frames`` = upper bound of the weights being injected (the number of frames that state carries); without it the
        volume no longer qualifies for the packed exchange form (the bound is unknown), halo copies excepted (they are
        never summed)."""
        n = int(keys.shape[0])
        _lib.check(self._lib.gs2m_tsdf_unpack(self._h, _ptr(keys), n, int(form), _ptr(buf_f32), _ptr(buf_i64),
                                              int(bool(halo)), _stream_of(keys, stream)), self._lib)
        if halo:
            self.has_halo = self.has_halo or n > 0
        else:
            self._inherit(frames)

    def replace(self, keys, form, buf_f32, buf_i64=None, stream=None, frames=None):
        """``gs2m_tsdf_replace``: reset + unpack of the DISTINCT blocks ``keys`` in one call (the reduced blocks' bytes are
        written once, not cleared first)."""
        n = int(keys.shape[0])
        _lib.check(self._lib.gs2m_tsdf_replace(self._h, _ptr(keys), n, int(form), _ptr(buf_f32), _ptr(buf_i64),
                                               _stream_of(keys, stream)), self._lib)
        self._reset_bookkeeping()
        self._inherit(frames, reduced=True)

    def _inherit(self, frames, reduced=False):
        """``reduced``: the state comes out of reduce_volume (bounded by the total of the reduction; the ranks' parts are
        disjoint or identical copies of ONE reduced volume).  Otherwise it is caller-injected state: counted like frames
        integrated here -- it adds up across ranks."""
        bound = int(frames) if frames is not None else _lib.XFORM_PACKED_MAX_FRAMES + 1
        if reduced:
            self.frames_base = max(self.frames_base, bound)
        else:
            # unpack REPLACES the state of the blocks it names (k_tsdf_unpack), so within ONE volume the bounds of several
            # calls do not add up -- a checkpoint loaded in chunks stays bounded by its frame count; what adds up
            # is the injected state of DIFFERENT ranks (one checkpoint loaded everywhere), and gs2mesh_amd.parallel sums
            # `frames_injected` across the ranks for exactly that reason
            self.frames_injected = max(self.frames_injected, bound)

    def flags_device(self, out, stream=None):
        """``gs2m_tsdf_flags_device``: the overflow flag word of `status` into the device int32 tensor ``out`` [1], async."""
        _lib.check(self._lib.gs2m_tsdf_flags_device(self._h, _ptr(out), _stream_of(out, stream)), self._lib)

    def pack_sum(self, keys, buf, stream=None):
        """``gs2m_tsdf_pack_sum``: accumulators of the blocks ``keys`` [n,3] in sum form -> ``buf`` [n,5,4096] f32."""
        n = int(keys.shape[0])
        _lib.check(self._lib.gs2m_tsdf_pack_sum(self._h, _ptr(keys), n, _ptr(buf), _stream_of(keys, stream)), self._lib)

    def unpack_sum(self, keys, buf, halo=False, stream=None, frames=None):
        """``gs2m_tsdf_unpack_sum``: replace the state of the blocks ``keys`` by ``buf`` (tsdf = wsum / weight);
        ``halo`` = neighbour-only blocks (read by the mesh extraction, never the base of a cube); ``frames`` as in `unpack`."""
        n = int(keys.shape[0])
        _lib.check(self._lib.gs2m_tsdf_unpack_sum(self._h, _ptr(keys), n, _ptr(buf), int(bool(halo)),
                                                  _stream_of(keys, stream)), self._lib)
        if halo:
            self.has_halo = self.has_halo or n > 0
        else:
            self._inherit(frames)
