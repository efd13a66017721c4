"""PNG files of the Renderer's stereo pairs made on the device (``gs2m_png_encode``), and a writer thread that puts them on disk.

``PngEncoder`` turns u8 RGB images on the device into complete PNG files on the device (the stream is described in
``include/gs2mesh_amd.h`` at ``gs2m_png_encode``); only the compressed bytes cross to the host.  ``PngWriter`` writes them from
a thread of its own: ``submit`` enqueues the encode and returns; the thread waits for it, copies the compressed bytes into pinned
host memory and writes ``path + ".tmp"``, renamed over ``path``, so a ``--skip_rendering`` resume never sees half a file.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading

import numpy as np

from . import _lib

try:  # torch is plumbing for device memory / streams; the emulator tests run without a device
    import torch
except Exception:  # pragma: no cover
    torch = None

FILTER_NONE, FILTER_PAETH = 0, 4


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _batch(rgb8):
    """[n,H,W,3] or [H,W,3] u8 -> contiguous [n,H,W,3]"""
    x = rgb8 if rgb8.ndim == 4 else rgb8[None]
    if x.ndim != 4 or x.shape[-1] != 3:
        raise ValueError(f"rgb8 must be [n,H,W,3] or [H,W,3] u8, got shape {tuple(rgb8.shape)}")
    if _is_torch(x):
        if x.dtype != torch.uint8:
            raise TypeError(f"rgb8 must be uint8, got {x.dtype}")
        return x.contiguous()
    if x.dtype != np.uint8:
        raise TypeError(f"rgb8 must be uint8, got {x.dtype}")
    return np.ascontiguousarray(x)


def _stream_handle(x, stream):
    if stream is not None:
        return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
    if _is_torch(x) and x.is_cuda:
        return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    return C.c_void_p(0)


def write_file(path: str, data) -> None:
    """``data`` to ``path`` through ``path + ".tmp"`` and a rename: readers see the old file or the whole new one."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


class PngEncoder:
    """Owns one ``gs2m_png`` handle (grow-only scratch).  One stream at a time.  ``lib``: another build of the C ABI
    (the tests pass the CPU-emulator build of the same kernel source)."""

    def __init__(self, device: int = 0, lib=None, rows_per_segment: int = 16, filter: int = FILTER_PAETH):
        self._lib = lib or _lib.get()
        h = C.c_void_p()
        _lib.check(self._lib.gs2m_png_create(C.byref(h), int(device)), self._lib)
        self._h = h
        self.device = int(device)
        self.rows_per_segment = int(rows_per_segment)
        self.filter = int(filter)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gs2m_png_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_bytes(self, width: int, height: int) -> int:
        """Upper bound of one file of ``width`` x ``height`` (every segment stored)."""
        v = int(self._lib.gs2m_png_max_bytes(int(width), int(height), self.rows_per_segment))
        if v < 0:
            raise ValueError(f"cannot encode a {width} x {height} PNG with rows_per_segment {self.rows_per_segment}")
        return v

    def encode_device(self, rgb8, stream=None):
        """Enqueue the encode of ``rgb8`` ([n,H,W,3] or [H,W,3] u8 on the device); no host synchronisation.  Returns
        (out [n, max_bytes] u8, nbytes [n] int64), both on the device: file k is ``out[k, :nbytes[k]]``."""
        x = _batch(rgb8)
        n, H, W, _ = x.shape
        stride = self.max_bytes(W, H)
        mem = _lib.MEMORY
        if _is_torch(x) and x.is_cuda:
            out = torch.empty((n, stride), dtype=torch.uint8, device=x.device)
            nbytes = torch.empty(n, dtype=torch.int64, device=x.device)
        else:
            out = mem.zeros((n, stride), np.uint8, self.device)
            nbytes = mem.zeros((n,), np.int64, self.device)
        _lib.check(self._lib.gs2m_png_encode(self._h, n, W, H, mem.ptr(x, name="rgb8"), H * W * 3, mem.ptr(out, name="out"),
                                             stride, mem.ptr(nbytes, name="nbytes"), self.filter, self.rows_per_segment,
                                             _stream_handle(x, stream)), self._lib)
        return out, nbytes

    def encode(self, rgb8, stream=None) -> list[bytes]:
        """The PNG files of ``rgb8`` ([n,H,W,3] or [H,W,3] u8 on the device), one ``bytes`` per image.  Synchronises."""
        out, nbytes = self.encode_device(rgb8, stream)
        if not _is_torch(out):
            return [out[k, :int(nbytes[k])].tobytes() for k in range(out.shape[0])]
        return self._download(out, nbytes, stream).wait()

    def encode_into(self, rgb8, stream=None) -> "PendingPng":
        """Asynchronous ``encode``: enqueues the encode and the copy of the file sizes into pinned memory and returns.
        ``.wait()`` copies the compressed bytes into pinned host memory and returns the files."""
        out, nbytes = self.encode_device(rgb8, stream)
        if not _is_torch(out):
            raise RuntimeError("encode_into needs device tensors")
        return self._download(out, nbytes, stream)

    def _download(self, out, nbytes, stream):
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        sizes = torch.empty(nbytes.shape, dtype=torch.int64, pin_memory=True)
        with torch.cuda.stream(s):
            sizes.copy_(nbytes, non_blocking=True)
            done = torch.cuda.Event()
            done.record(s)
        return PendingPng(out, sizes, done)


class PendingPng:
    """Files of one ``PngEncoder.encode_into`` call.  ``wait()`` blocks until they are on the host (any thread)."""

    def __init__(self, out, sizes, done):
        self._out, self._sizes, self._done = out, sizes, done

    def wait(self) -> list[bytes]:
        self._done.synchronize()                    # encode + size copy complete
        sizes = [int(s) for s in self._sizes.tolist()]
        dev = self._out.device
        host = torch.empty(max(sum(sizes), 1), dtype=torch.uint8, pin_memory=True)
        copy = torch.cuda.Stream(device=dev)
        with torch.cuda.device(dev), torch.cuda.stream(copy):
            o = 0
            for k, s in enumerate(sizes):           # only the compressed bytes leave the device
                host[o:o + s].copy_(self._out[k, :s], non_blocking=True)
                o += s
        copy.synchronize()
        buf = host.numpy()
        files, o = [], 0
        for s in sizes:
            files.append(buf[o:o + s].tobytes())
            o += s
        self._out = None
        return files


class PngWriter:
    """Writes the files of ``submit(paths, rgb8)`` from a thread of its own.  At most ``max_pending`` batches are in flight
    (their device outputs and pinned host copies are what it holds); ``submit`` blocks beyond that.  ``flush()`` returns when
    every submitted file is on disk and re-raises the first write error; ``submit`` after an error raises too.  Parent
    directories are the caller's to create."""

    def __init__(self, encoder: PngEncoder, max_pending: int = 8):
        if max_pending < 1:
            raise ValueError("max_pending must be >= 1")
        self.encoder = encoder
        self._slots = threading.BoundedSemaphore(int(max_pending))
        self._jobs = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._run, name="gs2m-png-writer", daemon=True)
        self._thread.start()

    def submit(self, paths, rgb8, stream=None):
        if self._error is not None:
            raise RuntimeError(f"PngWriter: an earlier write failed: {self._error!r}") from self._error
        paths = [os.fspath(p) for p in paths]
        n = rgb8.shape[0] if rgb8.ndim == 4 else 1
        if len(paths) != n:
            raise ValueError(f"{len(paths)} paths for {n} images")
        self._slots.acquire()
        try:
            pending = self.encoder.encode_into(rgb8, stream)
        except BaseException:
            self._slots.release()
            raise
        self._jobs.put((paths, pending))

    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            try:
                paths, pending = job
                files = pending.wait()
                if self._error is None:
                    for path, data in zip(paths, files):
                        write_file(path, data)
            except BaseException as e:   # reported by flush() / the next submit()
                if self._error is None:
                    self._error = e
            finally:
                self._slots.release()
                self._jobs.task_done()

    def flush(self):
        self._jobs.join()
        if self._error is not None:
            raise self._error

    def close(self):
        if self._thread.is_alive():
            self._jobs.put(None)
            self._thread.join()
