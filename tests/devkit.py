"""Device memory for the tests of the device-resident entry points, through the library's own helpers (kvzx_harness_alloc / _upload / _download / _free):
a buffer that is allocated, written, read back and freed, and the download of a pitched plane -- what kvzx_decoder_output_device describes.  Test
infrastructure; nothing here knows the encoder or the decoder."""
import ctypes as C

import numpy as np


def bind(lib):
    if getattr(lib, "_devkit_bound", False):
        return lib
    lib.kvzx_harness_alloc.restype = C.c_void_p
    lib.kvzx_harness_alloc.argtypes = [C.c_int, C.c_size_t]
    lib.kvzx_harness_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.kvzx_harness_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.kvzx_harness_free.argtypes = [C.c_void_p]
    lib.kvzx_harness_sync.argtypes = [C.c_int]
    lib.kvzx_harness_synth_frame.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int]
    lib._devkit_bound = True
    return lib


class DeviceBuffer:
    """nbytes of device memory on device 0; data (optional) is uploaded at once"""

    def __init__(self, lib, nbytes, data=None):
        self.lib, self.nbytes = bind(lib), int(nbytes)
        self.ptr = lib.kvzx_harness_alloc(0, self.nbytes)
        assert self.ptr, "kvzx_harness_alloc(%d) failed" % self.nbytes
        if data is not None:
            self.upload(data)

    def upload(self, data):
        """the whole array to the start of the buffer; the copy has completed when this returns"""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        assert self.ptr and data.nbytes <= self.nbytes, (data.nbytes, self.nbytes)
        assert self.lib.kvzx_harness_upload(self.ptr, data.ctypes.data, data.nbytes), "kvzx_harness_upload failed"
        assert self.lib.kvzx_harness_sync(0)

    def download(self, nbytes=None):
        assert self.ptr
        return download(self.lib, self.ptr, self.nbytes if nbytes is None else nbytes)

    def free(self):
        if self.ptr:
            self.lib.kvzx_harness_free(self.ptr)
            self.ptr = None


def download(lib, ptr, nbytes):
    """nbytes from the device address ptr"""
    out = np.empty(int(nbytes), dtype=np.uint8)
    assert bind(lib).kvzx_harness_download(out.ctypes.data, ptr, out.nbytes), "kvzx_harness_download failed"
    return out


def download_plane(lib, ptr, pitch, width, height):
    """a pitched plane in device memory, cut to width x height: ONE copy of the rows' span (the last row ends at its width: not a byte is read behind
    what the plane's owner describes)"""
    assert ptr and pitch >= width > 0 and height > 0, (ptr, pitch, width, height)
    span = download(lib, ptr, pitch * (height - 1) + width)
    rows = np.zeros(pitch * height, dtype=np.uint8)
    rows[:span.size] = span
    return rows.reshape(height, pitch)[:, :width].copy()


def download_i420(lib, planes, pitches, width, height):
    """the three planes of kvzx_decoder_output_device as one packed I420 picture of width x height"""
    return np.concatenate([download_plane(lib, planes[c], pitches[c], width >> (c > 0), height >> (c > 0)).reshape(-1) for c in range(3)])


def synth_clip(lib, kind, seed, w, h, n):
    """n pictures of the synthetic clip generated in device memory (kvzx_harness_synth_frame), one buffer each"""
    bufs = []
    for t in range(n):
        b = DeviceBuffer(lib, w * h * 3 // 2)
        assert lib.kvzx_harness_synth_frame(b.ptr, kind, seed, w, h, t), "kvzx_harness_synth_frame failed"
        bufs.append(b)
    assert lib.kvzx_harness_sync(0)
    return bufs
