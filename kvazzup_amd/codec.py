"""Thin Python drivers over the C ABI, used by tests/ and bench.py.  They perform exactly the
call sequences of uvgComm's filters (kvazaarfilter.cpp:145-299,407-476; openhevcfilter.cpp:36-56,
112-172,194-237); the C++ mirrors of those filters live in csrc/filters.hip."""
import ctypes as C
import numpy as np
from . import _native as N

DEFAULT_OPTIONS = (("preset", "ultrafast"), ("threads", "0"), ("owf", "0"), ("wpp", "1"), ("qp", "32"), ("period", "64"),
                   ("vps-period", "1"), ("intra-bits", ""), ("gop", "lp-g4d3t1"), ("scaling-list", "off"), ("mv-constraint", "none"))


class Encoder:
    """kvz_api driven the way KvazaarFilter::init / feedInput drive it."""

    def __init__(self, width, height, fps=(30, 1), options=(), fields=None):
        self.lib = N.load_library()
        self.api = self.lib.kvz_api_get(8).contents
        self.w, self.h = width, height
        self.cfg = self.api.config_alloc()
        if not self.cfg:
            raise RuntimeError("config_alloc failed")
        self.api.config_init(self.cfg)
        opts = dict(DEFAULT_OPTIONS)
        opts["input-res"] = "%dx%d" % (width, height)
        opts["input-fps"] = "%d/%d" % fps
        for k, v in options:
            opts[k] = str(v)
        self.rejected = []
        for k, v in opts.items():
            if self.api.config_parse(self.cfg, k.encode(), v.encode()) != 1:
                self.rejected.append(k)
        self.cfg.contents.target_bitrate = 0
        self.cfg.contents.hash = 0
        for k, v in (fields or {}).items():
            setattr(self.cfg.contents, k, v)
        self.enc = self.api.encoder_open(self.cfg)
        if not self.enc:
            self.api.config_destroy(self.cfg)
            self.cfg = None
            raise RuntimeError("kvz_api.encoder_open failed (no usable HIP device? there is no CPU fallback)")
        # the ring of input pictures KvazaarFilter keeps (createInputVector(owf + 1), getNextPic: kvazaarfilter.cpp:32-42,76-88): the encoder
        # reads a picture where it lies until its access unit has come back, so a picture is not written again before that
        self.pics = [self.api.picture_alloc(width, height) for _ in range(int(self.cfg.contents.owf) + 1)]
        self.next_pic = 0
        self.pts = 0
        self._au = np.empty(width * height * 3 + (1 << 20), dtype=np.uint8)

    @property
    def pic(self):
        """the kvz_picture the next encode() call fills and hands over (tests set its roi fields, as KvazaarFilter::feedInput does)"""
        return self.pics[self.next_pic]

    # -- the reference call sequence: memcpy into kvz_picture, encoder_encode, drain chunks
    def encode(self, i420, want_recon=True):
        """i420 = None flushes (pic_in == NULL).  Returns (None, None) when the call produced no output
        (owf >= 1: the first call, or a flush with nothing in flight)."""
        ny = self.w * self.h
        if i420 is not None:
            i420 = np.ascontiguousarray(i420, dtype=np.uint8)
            pic = self.pics[self.next_pic]
            self.next_pic = (self.next_pic + 1) % len(self.pics)
            p = pic.contents
            C.memmove(p.y, i420.ctypes.data, ny)
            C.memmove(p.u, i420.ctypes.data + ny, ny // 4)
            C.memmove(p.v, i420.ctypes.data + ny + ny // 4, ny // 4)
            p.pts = self.pts
            self.pts += 1
        chunks = C.POINTER(N.KvzDataChunk)()
        length = C.c_uint32(0)
        recon = C.POINTER(N.KvzPicture)()
        info = N.KvzFrameInfo()
        ok = self.api.encoder_encode(self.enc, pic if i420 is not None else None, C.byref(chunks), C.byref(length),
                                     C.byref(recon) if want_recon else None, None, C.byref(info))
        if not ok:
            raise RuntimeError("encoder_encode failed")
        if not chunks:
            return None, None
        parts = []
        c = chunks
        while c:
            parts.append(bytes(c.contents.data[:c.contents.len]))
            c = c.contents.next
        self.api.chunk_free(chunks)
        au = b"".join(parts)
        assert len(au) == length.value
        rec = None
        if want_recon and recon:
            r = recon.contents
            rec = np.concatenate([np.frombuffer((C.c_char * n).from_address(ptr), dtype=np.uint8).copy()
                                  for ptr, n in ((r.y, ny), (r.u, ny // 4), (r.v, ny // 4))])
            self.api.picture_free(recon)
        self.info = {"poc": info.poc, "qp": info.qp, "nal_unit_type": info.nal_unit_type, "slice_type": info.slice_type,
                     "ref_list": [int(info.ref_list[0][k]) for k in range(int(info.ref_list_len[0]))]}
        return au, rec

    # -- extension entry points
    def encode_device(self, dptr):
        n = C.c_uint32(0)
        info = N.KvzFrameInfo()
        ok = self.lib.kvzx_encoder_encode_device(self.enc, dptr, self._au.ctypes.data, len(self._au), C.byref(n), C.byref(info))
        if not ok:
            raise RuntimeError("kvzx_encoder_encode_device failed")
        return bytes(self._au[:n.value])

    # -- "input-format" rgb32 / rgb32-sse41 / yuyv: the picture as one packed block, converted in the encoder's input stage
    def packed_bytes(self):
        """bytes of one input picture in the encoder's format"""
        return self.w * self.h * (3, 8, 8, 4)[int(self.cfg.contents.input_format)] // 2

    def _packed_out(self, ok, n, info, want_recon, what):
        if not ok:
            raise RuntimeError("%s failed" % what)
        if not n.value:
            return None, None
        self.info = {"poc": info.poc, "qp": info.qp, "nal_unit_type": info.nal_unit_type, "slice_type": info.slice_type,
                     "ref_list": [int(info.ref_list[0][k]) for k in range(int(info.ref_list_len[0]))]}
        rec = None
        if want_recon:
            ny = self.w * self.h
            rec = np.empty(ny * 3 // 2, dtype=np.uint8)
            if not self.lib.kvzx_encoder_download_recon(self.enc, rec.ctypes.data, rec.ctypes.data + ny, rec.ctypes.data + ny + ny // 4):
                raise RuntimeError("kvzx_encoder_download_recon failed")
        return bytes(self._au[:n.value]), rec

    def encode_packed(self, buf, want_recon=True):
        """a packed host picture (uint8, packed_bytes() long); None flushes.  Returns (access unit, reconstruction) like encode(), (None, None)
        when the call produced no output"""
        if buf is not None:
            buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
            if buf.size != self.packed_bytes():
                raise ValueError("a packed picture of %d bytes, the encoder's format has %d" % (buf.size, self.packed_bytes()))
        n = C.c_uint32(0)
        info = N.KvzFrameInfo()
        ok = self.lib.kvzx_encoder_encode_packed_host(self.enc, buf.ctypes.data if buf is not None else None, self._au.ctypes.data, len(self._au), C.byref(n), C.byref(info))
        return self._packed_out(ok, n, info, want_recon, "kvzx_encoder_encode_packed_host")

    def encode_packed_device(self, dptr, want_recon=True):
        """the same for a packed picture in device memory (an address; None flushes)"""
        n = C.c_uint32(0)
        info = N.KvzFrameInfo()
        ok = self.lib.kvzx_encoder_encode_packed_device(self.enc, dptr, self._au.ctypes.data, len(self._au), C.byref(n), C.byref(info))
        return self._packed_out(ok, n, info, want_recon, "kvzx_encoder_encode_packed_device")

    def report_damage(self, poc, first_ctb, count):
        """"loss-feedback": the receiver's loss report (a triple of Decoder.damage_log()); 1 accepted -- the next picture is the heal picture --, 2 void, 0 refused"""
        return int(self.lib.kvzx_encoder_report_damage(self.enc, int(poc), int(first_ctb), int(count)))

    def coded_size(self):
        a, b = C.c_int(), C.c_int()
        self.lib.kvzx_encoder_coded_size(self.enc, C.byref(a), C.byref(b))
        return a.value, b.value

    def debug(self, what, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        if not self.lib.kvzx_encoder_debug_copy(self.enc, what.encode(), out.ctypes.data, out.nbytes):
            raise RuntimeError("debug_copy(%s) failed" % what)
        return out

    def debug_all(self):
        cw, ch = self.coded_size()
        b8 = (ch // 8, cw // 8)
        d = {"coded_w": cw, "coded_h": ch}
        for k in ("cu_log2", "cu_intra", "cu_flags", "cu_merge_idx", "cu_mvp_idx", "cu_intra_mode", "cu_cbf"):
            d[k] = self.debug(k, np.uint8, b8)
        d["cu_mv"] = self.debug("cu_mv", np.int16, b8 + (2,))
        # ref_idx_l0 per 8x8 block: an array of its own only with lp-refs >= 2, else every block refers to reference 0
        d["cu_ref"] = np.zeros(b8, dtype=np.uint8)
        self.lib.kvzx_encoder_debug_copy(self.enc, b"cu_ref", d["cu_ref"].ctypes.data, d["cu_ref"].nbytes)
        # me-coarse: the centres the coarse stage gave the picture's 32x32 blocks, (x, y) in full samples per reference -- a key of its own only with the option on
        if int(self.cfg.contents.me_coarse):
            d["me_coarse"] = self.debug("me_coarse", np.int16, (4, ch // 32, cw // 32, 2))
        # lp-gop: what the encoder planned for the picture -- its QP layer, QP and references (POC distances in list 0 order) -- a key of its own only with the option on
        if int(self.cfg.contents.lp_gop):
            g = self.debug("lp_gop", np.int32, (8,))
            d["lp_gop"] = {"active": int(g[0]), "layer": int(g[1]), "qp": int(g[2]), "dists": [int(v) for v in g[4:4 + int(g[3])]]}
        # weightp: the luma weights the picture's slice headers carry, per reference in list 0 order -- a key of its own only with the option on
        if int(self.cfg.contents.weightp):
            d["wp"] = self.debug("wp", np.int32, (4, 3))
        # intra-refresh: position in the cycle, the band's first and end column, the cycle's length -- a key of its own only with the option on
        if int(self.cfg.contents.intra_refresh):
            d["ir"] = [int(v) for v in self.debug("ir", np.int32, (4,))]
        # loss-feedback: the delivered picture's record, and the map and block records of the heal picture last submitted -- keys of their own only with the option on
        if int(self.cfg.contents.loss_feedback):
            d["fb"] = dict(zip(("heal", "reports", "cells", "forced"), (int(v) for v in self.debug("fb", np.int32, (4,)))))
            d["fb_map"] = self.debug("fb_map", np.uint8, b8)
            d["fb_blk"] = self.debug("fb_blk", np.uint8, (ch // 32, cw // 32, 2))
        # fb-anchor: the delivered picture's record -- a key of its own only with the option on ("cu_ref" above: a v2 heal picture's references, zero in every other picture)
        if int(self.cfg.contents.fb_anchor):
            d["fb_anchor"] = dict(zip(("v2", "anchor", "da", "ref1_quarters"), (int(v) for v in self.debug("fb_anchor", np.int32, (4,)))))
        # scenecut: the delivered picture's record, and (S, A) of every block of the picture last examined -- keys of their own only with the option on
        if int(self.cfg.contents.scenecut):
            d["scenecut"] = dict(zip(("examined", "n_new", "n_b", "d", "cut"), (int(v) for v in self.debug("scenecut", np.int32, (5,)))))
            d["sc_blocks"] = self.debug("sc_blocks", np.uint32, ((self.h + 31) // 32, (self.w + 31) // 32, 2))
        for c in range(3):
            shp = (ch, cw) if c == 0 else (ch // 2, cw // 2)
            d["coef%d" % c] = self.debug("coef%d" % c, np.int16, shp)
            d["rec%d" % c] = self.debug("rec%d" % c, np.uint8, shp)
            d["src%d" % c] = self.debug("src%d" % c, np.uint8, shp)
        return d

    def set_profiling(self, on):
        self.lib.kvzx_encoder_set_profiling(self.enc, int(on))

    def kernel_times(self, reset=True):
        ms = (C.c_double * 16)()
        n = (C.c_uint64 * 16)()
        k = self.lib.kvzx_encoder_kernel_times(self.enc, ms, n, int(reset))
        return {self.lib.kvzx_encoder_kernel_name(i).decode(): (ms[i], n[i]) for i in range(k)}

    def last_bins(self):
        return self.lib.kvzx_encoder_last_bins(self.enc)

    def close(self):
        if getattr(self, "enc", None):
            self.api.encoder_close(self.enc)
            self.enc = None
        for pic in getattr(self, "pics", []):
            self.api.picture_free(pic)
        self.pics = []
        if getattr(self, "cfg", None):
            self.api.config_destroy(self.cfg)
            self.cfg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_nals(au):
    """Annex-B access unit -> list of NAL units, each with its 4-byte start code (what uvgRTP hands to
    OpenHEVCFilter one by one, /root/reference/src/media/delivery/uvgrtpreceiver.cpp:86-112)."""
    au = bytes(au)
    starts = []
    i = 0
    while True:
        j = au.find(b"\x00\x00\x00\x01", i)
        if j < 0:
            break
        starts.append(j)
        i = j + 4
    starts.append(len(au))
    return [au[starts[k]:starts[k + 1]] for k in range(len(starts) - 1)]


class Decoder:
    """libOpenHevc* driven the way OpenHEVCFilter::init / process / sendDecodedOutput drive it."""

    OH_THREAD_FRAME, OH_THREAD_SLICE = 1, 2

    def __init__(self, threads=1, download=True, device=None, frame_threads=False, temporal_layer=7, no_cropping=False, concealment=2, partial_pictures=False):
        """concealment: what stands in for a lost reference picture -- 2 a copy of the nearest one, 3 that picture moved along its own motion (kvazzup_amd.h
        kvzx_decoder_set_concealment); partial_pictures: a picture that lost slice segments keeps what arrived (kvzx_decoder_set_partial_pictures) -- every
        picture handed out then carries "missing_ctbs" and "total_ctbs" """
        self.lib = N.load_library()
        self.threads, self.frame_threads = threads, bool(frame_threads) and threads > 1
        self.h = self.lib.libOpenHevcInit(threads, self.OH_THREAD_FRAME if frame_threads else self.OH_THREAD_SLICE)
        if device is not None:
            self.lib.kvzx_decoder_set_device(self.h, device)
        if concealment != 2 and not self.set_concealment(concealment):
            self.lib.libOpenHevcClose(self.h)
            self.h = None
            raise ValueError("concealment mode %r (2 or 3)" % (concealment,))
        self.partial_pictures = bool(partial_pictures)
        if partial_pictures and not self.lib.kvzx_decoder_set_partial_pictures(self.h, 1):
            self.lib.libOpenHevcClose(self.h)
            self.h = None
            raise ValueError("partial pictures were refused")
        if self.lib.libOpenHevcStartDecoder(self.h) == -1:
            self.lib.libOpenHevcClose(self.h)
            self.h = None
            raise RuntimeError("libOpenHevcStartDecoder failed (no usable HIP device? there is no CPU fallback)")
        self.lib.libOpenHevcSetTemporalLayer_id(self.h, int(temporal_layer))      # (the highest sub-layer decoded: OpenHEVC's default 7 = all; uvgComm's filter passes 0, openhevcfilter.cpp:54)
        self.lib.libOpenHevcSetActiveDecoders(self.h, 0)
        if no_cropping:
            self.lib.libOpenHevcSetNoCropping(self.h, 1)                # (pictures at their coded size: the conformance window is not applied)
        self.lib.libOpenHevcSetViewLayers(self.h, 0)
        self.download = download
        if not download:
            self.lib.kvzx_decoder_set_download(self.h, 0)
        self.vps = self.sps = self.pps = False

    def decode_nal(self, nal, pts=0):
        """returns None or a dict with the packed I420 picture (the row-wise copy of sendDecodedOutput)"""
        nal = bytes(nal)
        if len(nal) < 6:                     # not a NAL unit (csrc/filters.hip OpenHEVCFilter::process drops it the same way)
            return None
        t = nal[4] >> 1
        self.vps |= t == 32
        self.sps |= t == 33
        self.pps |= t == 34
        vcl = t <= 31
        if not ((self.vps and self.sps and self.pps) or not vcl):
            return None
        buf = (C.c_ubyte * len(nal)).from_buffer_copy(nal)
        got = self.lib.libOpenHevcDecode(self.h, buf, len(nal), pts)
        if got < 0:
            raise RuntimeError("libOpenHevcDecode error %d" % got)
        if got == 0:
            return None
        fr = N.OpenHevcFrame()
        if self.lib.libOpenHevcGetOutput(self.h, got, C.byref(fr)) <= 0:
            return None
        self.lib.libOpenHevcGetPictureInfo(self.h, C.byref(fr.frameInfo))
        info = fr.frameInfo
        w, h = info.nWidth, info.nHeight
        out = {"width": w, "height": h, "fps": (info.frameRate.num, info.frameRate.den), "pts": info.nTimeStamp}
        if getattr(self, "partial_pictures", False):                # (tests build a Decoder around a handle of their own, without __init__)
            missing, total = C.c_int(), C.c_int()
            if self.lib.kvzx_decoder_damage(self.h, C.byref(missing), C.byref(total)):
                out["missing_ctbs"], out["total_ctbs"] = missing.value, total.value
        if self.download:
            ys, qs = info.nYPitch, info.nUPitch // 2
            y = np.empty((h, w), np.uint8)
            u = np.empty((h // 2, w // 2), np.uint8)
            v = np.empty((h // 2, w // 2), np.uint8)
            for i in range(h):                              # openhevcfilter.cpp:218-229
                y[i] = np.frombuffer((C.c_char * w).from_address(fr.pvY + i * ys), dtype=np.uint8)
                if i % 2 == 0:
                    u[i // 2] = np.frombuffer((C.c_char * (w // 2)).from_address(fr.pvU + i * qs), dtype=np.uint8)
                    v[i // 2] = np.frombuffer((C.c_char * (w // 2)).from_address(fr.pvV + i * qs), dtype=np.uint8)
            out["i420"] = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
        return out

    def decode_au(self, au, pts=0):
        return [f for f in (self.decode_nal(n, pts) for n in split_nals(au)) if f is not None]

    def drain(self):
        """end-of-sequence NAL units hand out the pictures still held back: by the frame threads' ring, and -- a stream whose SPS allows
        reordering (B pictures in groups) -- by the output process, which lets go of them in POC order"""
        out = []
        ring = (self.threads + 1) if self.frame_threads else 1
        eos = bytes([0, 0, 0, 1, 36 << 1, 1])
        misses = 0
        for _ in range(ring + 20):                  # (ring + sps_max_num_reorder_pics <= 15 + slack)
            f = self.decode_nal(eos)
            if f is not None:
                out.append(f)
                misses = 0
            else:
                misses += 1
                if misses > ring:
                    break
        return out

    def set_concealment(self, mode):
        """False: refused (a mode other than 2 and 3, or the first picture has been decoded)"""
        return bool(self.lib.kvzx_decoder_set_concealment(self.h, int(mode)))

    def damage_log(self):
        """[(POC, first coding tree block, count)] of every damaged picture so far, in decoding order (partial_pictures)"""
        n = self.lib.kvzx_decoder_damage_log(self.h, None, 0)
        buf = (C.c_int32 * (3 * max(n, 1)))()
        n = min(n, self.lib.kvzx_decoder_damage_log(self.h, buf, n))
        return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]

    def fill_mv(self, w, h):
        """partial pictures: the displacements the last fill used, laid out like standin()'s table; None before the first one"""
        mv = np.empty(((h + 15) // 16, (w + 15) // 16, 4), np.int16)
        return mv if self.lib.kvzx_decoder_debug_copy(self.h, b"fill_mv", mv.ctypes.data, mv.nbytes) else None

    def standin(self, w, h):
        """concealment 3: the stand-in filled last, (Y, Cb, Cr) at the coded size w x h, and its displacements [ceil(h / 16)][ceil(w / 16)][4]
        (luma dx, dy, chroma dx, dy); None before the first one"""
        pw, ph = (w + 63) & ~63, (h + 63) & ~63
        buf = np.empty(pw * ph * 3 // 2, np.uint8)
        mv = np.empty(((h + 15) // 16, (w + 15) // 16, 4), np.int16)
        if not self.lib.kvzx_decoder_debug_copy(self.h, b"standin", buf.ctypes.data, buf.nbytes) or not self.lib.kvzx_decoder_debug_copy(self.h, b"standin_mv", mv.ctypes.data, mv.nbytes):
            return None
        y = buf[:pw * ph].reshape(ph, pw)[:h, :w]
        u = buf[pw * ph:pw * ph * 5 // 4].reshape(ph // 2, pw // 2)[:h // 2, :w // 2]
        v = buf[pw * ph * 5 // 4:].reshape(ph // 2, pw // 2)[:h // 2, :w // 2]
        return (y.copy(), u.copy(), v.copy()), mv

    def output_device(self):
        planes = (C.c_void_p * 3)()
        pitches = (C.c_int * 3)()
        if not self.lib.kvzx_decoder_output_device(self.h, planes, pitches):
            return None
        return list(planes), list(pitches)

    def set_output_hold(self, pictures):
        """download=False: the planes of output_device() stay untouched while this many further pictures are begun (kvzx_decoder_set_output_hold: 1..8, default 2)"""
        self.lib.kvzx_decoder_set_output_hold(self.h, int(pictures))

    def output_rgb32_device(self, d_rgb32, variant=0):
        """the picture handed out last, converted where it lies into width * height * 4 bytes at the device address d_rgb32"""
        return bool(self.lib.kvzx_decoder_output_rgb32_device(self.h, d_rgb32, int(variant)))

    def set_profiling(self, on):
        self.lib.kvzx_decoder_set_profiling(self.h, int(on))

    def kernel_times(self, reset=True):
        ms = (C.c_double * 16)()
        n = (C.c_uint64 * 16)()
        k = self.lib.kvzx_decoder_kernel_times(self.h, ms, n, int(reset))
        return {self.lib.kvzx_decoder_kernel_name(i).decode(): (ms[i], n[i]) for i in range(k)}

    def close(self):
        if getattr(self, "h", None):
            self.lib.libOpenHevcFlush(self.h)
            self.lib.libOpenHevcClose(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
