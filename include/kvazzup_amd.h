/*
 * include/kvazzup_amd.h -- extensions next to the two drop-in ABIs (kvazaar.h, openHevcWrapper.h):
 * device-resident entry points used by bench.py (inputs already in HBM), per-kernel timing taken
 * with HIP events on the library's own stream, and debug read-back used by the parity tests.
 * uvgComm itself needs none of these; they exist because its boundary hands over host buffers
 * (/root/reference/src/media/processing/kvazaarfilter.cpp:410-418 memcpy into kvz_picture,
 * openhevcfilter.cpp:218-229 memcpy out of the decoder's frame).
 */
#ifndef KVAZZUP_AMD_EXT_H_
#define KVAZZUP_AMD_EXT_H_
#include "kvazaar.h"
#include "openHevcWrapper.h"
#ifdef __cplusplus
extern "C" {
#endif

KVZ_PUBLIC const char *kvzx_version(void);
/* number of HIP devices visible (0 when the runtime cannot be initialised); touches the GPU */
KVZ_PUBLIC int kvzx_device_count(void);

/* ---- encoder ---- */
/* Encode one picture given as packed I420 (width*height*3/2 bytes) in DEVICE memory of the
 * encoder's GPU.  The access unit is written to au_buf (host).  Returns 1 on success, 0 on
 * failure or when au_cap is too small (*len_out still receives the needed size). */
KVZ_PUBLIC int kvzx_encoder_encode_device(kvz_encoder *enc, const void *d_i420, uint8_t *au_buf, uint32_t au_cap,
                                          uint32_t *len_out, kvz_frame_info *info_out);
/* Same with host planes (stride = width), without going through kvz_picture / chunk lists. */
KVZ_PUBLIC int kvzx_encoder_encode_host(kvz_encoder *enc, const uint8_t *y, const uint8_t *u, const uint8_t *v,
                                        uint8_t *au_buf, uint32_t au_cap, uint32_t *len_out, kvz_frame_info *info_out);
/* Encoders opened with "input-format" rgb32 / rgb32-sse41 / yuyv (kvazaar.h kvz_config.input_format) take their pictures here, as ONE packed block:
 * RGB32 width * height * 4 bytes, rows top to bottom; YUYV width * height * 2 bytes (Y0 U Y1 V).  The block's length is implied by the encoder's format --
 * the caller vouches for it as it does for the planes of the calls above -- and a device block of RGB32 must start at a multiple of 16 bytes.  The picture
 * is converted on the GPU in the encoder's input stage; the stream is that of an i420 encoder fed the converted picture.  A host block that starts a
 * page-locked kvz_picture (picture_alloc of a size that holds it) is read in place by the copy engine and must then stay unchanged until its access unit
 * has come back; any other host block is copied before the call returns.  NULL returns the picture in flight (owf >= 1).  On an i420 encoder both return
 * 0, as the two calls above (and encoder_encode) do on a packed one. */
KVZ_PUBLIC int kvzx_encoder_encode_packed_host(kvz_encoder *enc, const void *packed, uint8_t *au_buf, uint32_t au_cap, uint32_t *len_out, kvz_frame_info *info_out);
KVZ_PUBLIC int kvzx_encoder_encode_packed_device(kvz_encoder *enc, const void *d_packed, uint8_t *au_buf, uint32_t au_cap, uint32_t *len_out, kvz_frame_info *info_out);
KVZ_PUBLIC int kvzx_encoder_coded_size(kvz_encoder *enc, int *coded_w, int *coded_h);
/* cropped reconstruction of the last coded picture into host planes (stride = width) */
KVZ_PUBLIC int kvzx_encoder_download_recon(kvz_encoder *enc, uint8_t *y, uint8_t *u, uint8_t *v);
/* device pointers (coded size, pitch = coded width [/2]) of the last reconstruction */
KVZ_PUBLIC int kvzx_encoder_recon_device(kvz_encoder *enc, const void **planes /*[3]*/);
/* debug read-back of an internal array of the last coded picture: "cu_log2", "cu_intra", "cu_flags",
 * "cu_merge_idx", "cu_mvp_idx", "cu_intra_mode", "cu_cbf" (one byte per 8x8 block), "cu_mv", "cu_mvd"
 * (two int16 per 8x8 block), "coef0".."coef2" (int16 planes), "rec0".."rec2", "src0".."src2" */
KVZ_PUBLIC int kvzx_encoder_debug_copy(kvz_encoder *enc, const char *what, void *dst, size_t bytes);
KVZ_PUBLIC void kvzx_encoder_set_profiling(kvz_encoder *enc, int every);   /* 0 off, 1 every picture, n every n-th picture */
#define KVZX_MAX_KERNELS 16
/* accumulated HIP-event time (ms) and launch count per kernel id since the last reset */
KVZ_PUBLIC int kvzx_encoder_kernel_times(kvz_encoder *enc, double *ms, uint64_t *launches, int reset);
KVZ_PUBLIC const char *kvzx_encoder_kernel_name(int id);       /* NULL past the last id */
KVZ_PUBLIC uint64_t kvzx_encoder_last_bins(kvz_encoder *enc);  /* CABAC bins of the last picture */
KVZ_PUBLIC int kvzx_encoder_pending(kvz_encoder *enc);         /* pictures handed in whose access unit has not been returned yet */

/* ---- decoder ---- */
/* Decode one NAL unit whose OUTPUT is wanted in device memory: like libOpenHevcDecode. */
/* select the HIP device ordinal; call between libOpenHevcInit and libOpenHevcStartDecoder (default 0,
 * or the environment variable KVAZZUP_AMD_DEVICE) */
KVZ_PUBLIC int kvzx_decoder_set_device(OpenHevc_Handle h, int device);
KVZ_PUBLIC int kvzx_decoder_last_error(OpenHevc_Handle h);
/* What stands in for a reference picture that never arrived (a lost access unit): mode 2 (default) a copy of the nearest reference picture the decoder holds,
 * mode 3 that picture moved block by block along its own motion, continued to the lost picture's place in time (whole samples) -- the
 * better guess under camera motion and scrolling, an opt-in because it can lose about 1 dB where moving objects are as small as a block.  Either way grey
 * when there is no picture to take, and the stand-in is never handed out.  Call before the first picture.  Returns 1, or 0 for any other mode, for a call
 * after the first picture and for mode 3 on a band decoder (kvzx_decoder_set_band, which in turn is refused in mode 3).
 * kvzx_decoder_debug_copy: "standin" = the buffer of the stand-in filled last (mode 3; Y | Cb | Cr, pitch = the coded width rounded up to 64),
 * "standin_mv" = its displacements, int16 [ceil(h / 16)][ceil(w / 16)][4]: luma dx, dy, chroma dx, dy. */
KVZ_PUBLIC int kvzx_decoder_set_concealment(OpenHevc_Handle h, int mode);
/* Partial pictures v1 (off by default): a picture that lost slice segments on the way is not thrown away -- the coding tree blocks that arrived
 * are decoded, the others are filled from the nearest reference picture the way kvzx_decoder_set_concealment says (2: copied, 3: moved along its motion), and the
 * picture is handed out in its turn and kept as a reference.  Built for one-tile pictures: the form a Kvazaar peer's slices=wpp sends (WPP, a dependent slice segment per CTU row: the
 * rows before the lost one stay) and every other cut, free slices with or without WPP (gaps anywhere); pictures with tiles keep today's behaviour.  Call before the first picture; returns 1, or 0 after the first picture and on a band decoder
 * (kvzx_decoder_set_band, which in turn is refused while this is on).
 * kvzx_decoder_damage: the picture of the last libOpenHevcGetOutput -- coding tree blocks that were filled in, and how many it has (0 missing: whole); what an
 * application needs to ask the sender for a refresh.  Returns 0 when there is no such picture.
 * kvzx_decoder_damage_log: the runs (POC, first coding tree block, count) of all damaged pictures so far, in decoding order, up to `cap` triples; returns how many there
 * are (also under kvzx_decoder_set_parse_only).
 * kvzx_decoder_debug_copy: "partial_layout" = four bytes per coding tree block of the damaged picture filed last -- before the first one, of the picture parsed last -- (missing, its ctu_tile byte, its ctu_nb byte or 0xff,
 * min(255, transform blocks)), "fill_mv" = the displacements used last, laid out like "standin_mv"; "take_backs" = uint32, pictures whose first segments looked complete, ended early and were
 * opened again so far. */
KVZ_PUBLIC int kvzx_decoder_set_partial_pictures(OpenHevc_Handle h, int on);
KVZ_PUBLIC int kvzx_decoder_damage(OpenHevc_Handle h, int *missing_ctbs, int *total_ctbs);
KVZ_PUBLIC int kvzx_decoder_damage_log(OpenHevc_Handle h, int32_t *triples, int cap);
/* Test / measurement hook, not a decoding mode: before libOpenHevcStartDecoder.  The decoder then runs its HOST half only (NAL units, parameter sets, slice
 * headers, the CABAC slice-data parser with `parse_threads` row threads), touches no device and never outputs a picture (libOpenHevcDecode returns 0 or an
 * error).  kvzx_decoder_parse_probe_stats: out5 = pictures parsed, transform blocks, level words, FNV-1a digest of everything the parser produced, 0;
 * parse_ms = time spent in the slice-data parser. */
KVZ_PUBLIC int kvzx_decoder_set_parse_only(OpenHevc_Handle h, int parse_threads);
KVZ_PUBLIC int kvzx_decoder_parse_probe_stats(OpenHevc_Handle h, uint64_t *out5, double *parse_ms);
/* with libOpenHevcSetCheckMD5(h, 1): decoded picture hash SEI messages (MD5 / checksum, H.265 D.2.19) compared so far and how many did not
 * match the picture as decoded (each mismatch also sets the last error to -4 and is said on stderr; the picture is still handed out) */
KVZ_PUBLIC void kvzx_decoder_hash_stats(OpenHevc_Handle h, int *checked, int *mismatch);
/* device pointers (pitch = coded width [/2]) of the picture returned by the last libOpenHevcGetOutput */
KVZ_PUBLIC int kvzx_decoder_output_device(OpenHevc_Handle h, const void **planes /*[3]*/, int *pitches /*[3]*/);
/* when 0, libOpenHevcDecode leaves the picture in HBM and libOpenHevcGetOutput returns NULL planes */
KVZ_PUBLIC void kvzx_decoder_set_download(OpenHevc_Handle h, int on);
/* Lifetime of the device planes of kvzx_decoder_output_device (download off): they belong to the decoder's picture buffer and stay
 * untouched -- read as a reference picture at most -- while the next `pictures` pictures are begun (default 2, 1..8; values outside are
 * clamped): from the libOpenHevcDecode call that handed the picture out until the call that takes the first NAL unit of the
 * (`pictures` + 1)-th picture after that call -- with any number of frame threads, whatever other NAL units come between.  At the end of a
 * stream every end-of-sequence / end-of-bitstream NAL unit counts like a picture's first: it moves the frame threads' ring on by one
 * picture.  After that the buffer may be reused.  A consumer that lags further must copy, or raise this.  A stream that reorders its
 * pictures for output is handed out as dense copies (pitch = width) with the same lifetime. */
KVZ_PUBLIC void kvzx_decoder_set_output_hold(OpenHevc_Handle h, int pictures);
KVZ_PUBLIC void kvzx_decoder_set_profiling(OpenHevc_Handle h, int every);
KVZ_PUBLIC int kvzx_decoder_kernel_times(OpenHevc_Handle h, double *ms, uint64_t *launches, int reset);
KVZ_PUBLIC const char *kvzx_decoder_kernel_name(int id);
KVZ_PUBLIC int kvzx_decoder_debug_copy(OpenHevc_Handle h, const char *what, void *dst, size_t bytes);
/* ---- several decoders in one process on one device (uvgComm: one OpenHEVCFilter per peer, filtergraph.cpp:561-589): their pictures are launched by
 * the device's submission layer, same kernels of different decoders' pictures as ONE launch (csrc/batch.h).  Statistics since the last reset:
 * sizes[n] = batches of n pictures (n = 0..8, 9 entries); per kernel (kvzx_batch_kernel_name: 4 of them) the profiled batches' time, launches and
 * pictures (profiling as set with kvzx_decoder_set_profiling on any of the decoders).  Returns the number of kernels. */
KVZ_PUBLIC int kvzx_batch_stats(int device, uint64_t *batches, uint64_t *pictures, uint64_t *sizes /*[9]*/, double *ms /*[4]*/, uint64_t *launches /*[4]*/, uint64_t *frames /*[4]*/, int reset);
KVZ_PUBLIC const char *kvzx_batch_kernel_name(int id);
/* measurement aid: while held, the submission layer launches nothing and the decoders' pictures pile up; releasing launches them in full batches */
KVZ_PUBLIC void kvzx_batch_hold(int device, int on);

/* ---- tile-row split of ONE picture over several encoders, one per GPU / process (BASELINE configs[4]).
 * Every encoder is opened with the same configuration plus "tiles" = 1xN and "band-row0" / "band-rows" (CTU rows, whole
 * tiles).  Per picture and rank: phase1 (input, decisions, reconstruction, vertical-edge deblocking of the band) ->
 * export_halo -> exchange with rank - 1 (gets `up`) and rank + 1 (gets `down`), e.g. RCCL send/recv of the two device
 * blocks -> import_halo (NULL where there is no neighbour) -> phase2 (horizontal edges incl. the band's boundary edges,
 * tokenizer, arithmetic coding): the band's substreams, back to back in buf with sizes[].  Rank 0 gathers all substreams in
 * picture order and calls kvzx_assemble_access_unit (host only).  kvazzup_amd/tilesplit.py drives this over torch.distributed. */
/* delta-QP map for the pictures submitted through the device entry point (the host entry point takes it from kvz_picture.roi,
 * kvazaarfilter.cpp:423-431): w x h int8 cells over the picture, w == 0 removes it; needs "set-qp-in-cu" = 1 */
KVZ_PUBLIC void kvzx_encoder_set_roi(kvz_encoder *enc, int w, int h, const int8_t *map);
/* "loss-feedback" = H ("uvgx loss feedback v1"): the receiver's loss report, the triples of kvzx_decoder_damage_log handed over unchanged.
 * poc names the MOST RECENTLY CODED picture with that POC; first_ctb and count are 64x64 coding tree blocks in raster order of the coded picture; count <= 0:
 * the whole picture -- an access unit that never arrived, or an application's "refresh now".  Returns
 *   1  accepted: the first picture handed in after the call returns is the heal picture -- a P picture with intra units where the error may have travelled,
 *      starting with a recovery point SEI; from it on the receiver has the encoder's pictures exactly.  Several reports before one picture fold into one heal
 *      picture; a report older than H pictures is accepted and treated as "everything damaged" (every quarter of the heal picture is intra);
 *   2  void: an IDR picture has been coded since the reported picture, there is nothing to heal and the stream is unchanged;
 *   0  refused: the option is off (a band encoder cannot have it on), or the range lies outside the picture.
 * A stale report whose POC collides with a newer picture of the same POC (behind a later IDR picture) is taken for that newer picture: it over-heals and never
 * under-heals.  Call it from the thread that hands pictures in, between any two of its calls; with owf >= 2 it waits until the encoder's submitter thread has
 * planned every picture handed in so far, and is safe against that thread. */
KVZ_PUBLIC int kvzx_encoder_report_damage(kvz_encoder *enc, int32_t poc, int first_ctb, int count);
/* Rate control ("bitrate" > 0) in band mode: every band's encoder runs the same picture-level controller, which books the size of access
 * unit t - 3 before picture t; the caller tells EVERY encoder the size of each assembled access unit (picture = 0, 1, ...) before
 * picture + 3 is started.  kvazzup_amd/tilesplit.py passes the sizes along with the substream headers it gathers anyway. */
KVZ_PUBLIC void kvzx_encoder_band_report_au(kvz_encoder *enc, long picture, uint32_t bytes);
KVZ_PUBLIC int kvzx_encoder_band_phase1(kvz_encoder *enc, const void *d_i420);
KVZ_PUBLIC size_t kvzx_encoder_band_halo_bytes(kvz_encoder *enc);
KVZ_PUBLIC int kvzx_encoder_band_export_halo(kvz_encoder *enc, void *d_up, void *d_down);
KVZ_PUBLIC int kvzx_encoder_band_import_halo(kvz_encoder *enc, const void *d_from_up, const void *d_from_down);
KVZ_PUBLIC int kvzx_encoder_band_phase2(kvz_encoder *enc, uint8_t *buf, uint32_t cap, uint32_t *sizes, int max_sub, int *nsub_out, kvz_frame_info *info);
/* The same in two halves, so that the halo exchange runs beside the first: 2a (inner horizontal edges, tokenizer, arithmetic coder) needs
 * nothing from the neighbouring bands and may be called BEFORE kvzx_encoder_band_import_halo; 2b (the band's two boundary edges) after it. */
KVZ_PUBLIC int kvzx_encoder_band_phase2a(kvz_encoder *enc);
KVZ_PUBLIC int kvzx_encoder_band_phase2b(kvz_encoder *enc, uint8_t *buf, uint32_t cap, uint32_t *sizes, int max_sub, int *nsub_out, kvz_frame_info *info);
KVZ_PUBLIC int kvzx_assemble_access_unit(const kvz_config *cfg, int idr, int poc, int write_parameter_sets, int slice_qp, const uint8_t *data,
                                          const uint32_t *sizes, int nsub, uint8_t *out, uint32_t cap, uint32_t *len_out);

/* ---- the decoding side of the tile-row split: one decoder per GPU / process, each reconstructing CTU rows [row0, row0 + nrows) (whole tile rows)
 * of a stream whose motion vectors stay inside their tiles (what the split encoder writes; no SAO, no temporal motion prediction; synchronous decoder).
 * Every decoder gets every NAL unit and parses its own rows' substreams only.  Per picture: libOpenHevcDecode (returns 0 once the band is
 * reconstructed) -> band_export(0, down) -> exchange: to rank + 1, from rank - 1 -> band_import(0, from_up) -> band_deblock -> band_export(1, up)
 * -> exchange: to rank - 1, from rank + 1 -> band_import(1, from_down) -> band_finish (> 0: the picture is the output, this band's rows of it valid).
 * Halo blocks are kvzx_decoder_band_halo_bytes() long, in device memory; the calls that have no neighbour on their side are skipped. */
KVZ_PUBLIC int kvzx_decoder_set_band(OpenHevc_Handle h, int row0, int nrows);          /* before the first picture */
KVZ_PUBLIC size_t kvzx_decoder_band_halo_bytes(OpenHevc_Handle h);                     /* after the first picture's parameter sets: 8 bytes per luma column */
KVZ_PUBLIC int kvzx_decoder_band_export(OpenHevc_Handle h, int stage, void *d_buf);
KVZ_PUBLIC int kvzx_decoder_band_import(OpenHevc_Handle h, int stage, const void *d_buf);
KVZ_PUBLIC int kvzx_decoder_band_ready(OpenHevc_Handle h);      /* 1: the band of a picture is reconstructed and waits for the exchange (after the picture's last slice segment) */
KVZ_PUBLIC int kvzx_decoder_band_deblock(OpenHevc_Handle h);
KVZ_PUBLIC int kvzx_decoder_band_finish(OpenHevc_Handle h);

/* ---- row f1: I420 -> RGB32, the conversion uvgComm runs on every decoded picture before display
 * (YUVtoRGB32::process, src/media/processing/yuvtorgb32.cpp:29-64 -> yuv420_to_rgb_i_{avx2_mt,avx2,sse41,c},
 * src/media/processing/yuvconversions.cpp:72-493).  The reference has two arithmetics; `variant` picks:
 *   0 = what the filter picks on an AVX2/SSE4.1 host: the SIMD arithmetic when width % 16 == 0, else the scalar one
 *   1 = yuv420_to_rgb_i_c (every fourth output byte left as found), 2 = the SIMD converters (fourth byte 0; width % 8 == 0)
 * Planes and output in device memory; returns 1 when the kernel was launched on `hip_stream`. */
KVZ_PUBLIC int kvzx_yuv420_to_rgb32_device(const void *d_y, const void *d_u, const void *d_v, int y_pitch, int c_pitch, void *d_rgb32,
                                            int width, int height, int variant, void *hip_stream);
/* host buffers in and out, like yuv420_to_rgb_i_*(input, output, width, height): upload, convert, download */
KVZ_PUBLIC int kvzx_yuv420_to_rgb32(const uint8_t *i420, uint8_t *rgb32, int width, int height, int variant);
/* the picture returned by the last libOpenHevcGetOutput, converted where it lies in HBM (no host copy); synchronous */
KVZ_PUBLIC int kvzx_decoder_output_rgb32_device(OpenHevc_Handle h, void *d_rgb32, int variant);

/* RGB32 -> I420, the converters of src/media/processing/yuvconversions.cpp:634-797, bit for bit (their quirks included: see
 * kvazzup_amd/csrc/color_kernels.hip).  variant 1 = rgb_to_yuv420_i_c, 2 = rgb_to_yuv420_i_sse41 (which turns the picture upside
 * down).  width % 4 == 0, height % 2 == 0.  Output: packed I420 (width * height * 3 / 2 bytes). */
KVZ_PUBLIC int kvzx_rgb32_to_yuv420_device(const void *d_rgb32, void *d_i420, int width, int height, int variant, void *hip_stream);
KVZ_PUBLIC int kvzx_rgb32_to_yuv420(const uint8_t *rgb32, uint8_t *i420, int width, int height, int variant);
/* measurement aid: `reps` launches of kvzx_rgb32_to_yuv420_device on the default stream, each timed with a pair of HIP events; ms_out[reps] */
KVZ_PUBLIC int kvzx_rgb32_to_yuv420_device_timed(const void *d_rgb32, void *d_i420, int width, int height, int variant, int reps, float *ms_out);

/* ---- filter-graph harness (kvazzup_amd/csrc/filters.h): KvazaarFilter -> [WireAdapter -> OpenHEVCFilter] ----
 * A Qt-free restatement of the two uvgComm filters on this path, each on its own thread with the
 * reference's input-buffer contract (src/media/processing/filter.cpp:151-222,364-417), driven through the
 * two ABIs above.  settings_text: "key=value" lines, key names of src/settingskeys.h:36-67 ("video/QP",
 * "video/Intra", "video/ResolutionWidth" ...) plus "uvgx/gpu", "uvgx/decoderDownload", "parameters/<i>/Name|Value". */
KVZ_PUBLIC void *uvgx_pipeline_create(const char *settings_text, int loopback_decode, int keep_outputs);
KVZ_PUBLIC int uvgx_pipeline_push_host(void *p, const uint8_t *i420, int w, int h, int fps_num, int fps_den, int64_t pts);
KVZ_PUBLIC int uvgx_pipeline_push_device(void *p, const void *d_i420, int w, int h, int fps_num, int fps_den, int64_t pts);
/* a packed RGB32 / YUYV picture (type: uvgx::DataType, DT_RGB32VIDEO = 1 << 10 or DT_YUYVVIDEO = 1 << 4) for a graph whose settings say
 * uvgx/inputFormat = rgb32 | rgb32-sse41 | yuyv: the encoder filter hands it over without a host conversion; 0 = rejected */
KVZ_PUBLIC int uvgx_pipeline_push_packed_host(void *p, const uint8_t *packed, int type, int w, int h, int fps_num, int fps_den, int64_t pts);
KVZ_PUBLIC int uvgx_pipeline_push_packed_device(void *p, const void *d_packed, int type, int w, int h, int fps_num, int fps_den, int64_t pts);
KVZ_PUBLIC int uvgx_pipeline_wait(void *p, uint64_t n_outputs, int timeout_ms);
/* push_device for a source that paces itself: sleeps until the encoder filter buffers fewer than max_backlog pictures (uvgComm filters
 * drop inputs at 10 buffered, filter.cpp:151-222); 0 = timed out or rejected */
KVZ_PUBLIC int uvgx_pipeline_push_device_paced(void *p, const void *d_i420, int w, int h, int fps_num, int fps_den, int64_t pts, uint32_t max_backlog, int timeout_ms);
/* the same for a HOST picture -- the reference's own boundary: the encoder filter copies it into a kvz_picture and calls encoder_encode
 * (kvazaarfilter.cpp:410-438).  borrow != 0: no copy into the Data object, the caller keeps i420 unchanged until the picture is encoded */
KVZ_PUBLIC int uvgx_pipeline_push_host_paced(void *p, const uint8_t *i420, int w, int h, int fps_num, int fps_den, int64_t pts, uint32_t max_backlog, int timeout_ms, int borrow);
KVZ_PUBLIC uint32_t uvgx_pipeline_encoder_backlog(void *p);
/* harness only (uvgComm never flushes a running graph): the pictures held back by video/OWF and by the decoder's frame threads
 * come out without further input -- the encoder filter runs its encoder_encode(NULL) loop to the end, the wire adapter sends
 * end-of-sequence NAL units.  The next picture pushed should be an IDR. */
KVZ_PUBLIC int uvgx_pipeline_flush(void *p);
KVZ_PUBLIC int uvgx_pipeline_pop_encoded(void *p, uint8_t *buf, uint32_t cap, uint32_t *size, int64_t *pts);
KVZ_PUBLIC int uvgx_pipeline_pop_decoded(void *p, uint8_t *buf, uint32_t cap, uint32_t *size, int *w, int *h, int64_t *pts);
KVZ_PUBLIC void uvgx_pipeline_stats(void *p, uint64_t *out8);
KVZ_PUBLIC void uvgx_pipeline_busy_ms(void *p, double *out3);   /* time inside process(): encoder, wire adapter, decoder filter */
KVZ_PUBLIC void uvgx_pipeline_avg_queue(void *p, double *out3); /* inputs found buffered by an arriving input, averaged: encoder, wire adapter, decoder filter */
/* per-picture delays in microseconds (what uvgComm's statistics window shows: kvazaarfilter.cpp:478-479 encoding delay, displayfilter.cpp:113-115 total
   delay).  which 0: picture pushed -> access unit out of the encoder filter; 1: -> decoded picture out of the last filter.  Returns the samples held since
   the last reset (up to `cap` copied, in output order). */
KVZ_PUBLIC uint32_t uvgx_pipeline_latency_us(void *p, int which, uint32_t *out, uint32_t cap, int reset);
KVZ_PUBLIC void uvgx_pipeline_delay_stats(void *p, double *out8);  /* the filters' own histograms: count, mean, p50, p99 of the encoding delay; the same of the total delay */
KVZ_PUBLIC void *uvgx_pipeline_encoder(void *p);     /* kvz_encoder* of the KvazaarFilter */
KVZ_PUBLIC void *uvgx_pipeline_decoder(void *p);     /* OpenHevc_Handle of the OpenHEVCFilter (NULL without loop-back) */
KVZ_PUBLIC void uvgx_pipeline_destroy(void *p);

/* ---- measurement harness (kvazzup_amd/csrc/harness_kernels.hip): the synthetic clip of SURVEY.md 8(d) generated in device memory, the buffers to
 * keep it in, a luma error sum -- so that bench.py needs no tensor library in the process (one that ships its own HIP runtime would replace the
 * system's for this library too).  Nothing of the codec. */
KVZ_PUBLIC void *kvzx_harness_alloc(int device, size_t bytes);           /* device memory; NULL on failure */
KVZ_PUBLIC void kvzx_harness_free(void *p);
KVZ_PUBLIC int kvzx_harness_sync(int device);                            /* hipDeviceSynchronize */
KVZ_PUBLIC int kvzx_harness_download(void *host, const void *dev, size_t bytes);
KVZ_PUBLIC int kvzx_harness_upload(void *dev, const void *host, size_t bytes);
/* uvgx-synth-v1 (kind 0 moving objects, 1 flat, 2 noise; kvazzup_amd/synth.py is the statement) as packed I420 into d_i420 (w*h*3/2 bytes) */
KVZ_PUBLIC int kvzx_harness_synth_frame(void *d_i420, int kind, uint32_t seed, int w, int h, int t);
/* sum of squared differences of the luma planes of a packed picture (pitch w) and a pitched one; < 0 on failure */
KVZ_PUBLIC double kvzx_harness_luma_sse(const void *d_a, const void *d_b, int w, int h, int pitch_b);
/* HBM peak in GB/s from the device properties (2 x memory clock x bus width / 8); 0 when the runtime does not report them */
KVZ_PUBLIC double kvzx_harness_hbm_peak_gbs(int device);
KVZ_PUBLIC int kvzx_harness_device_info(int device, char *name, int name_cap, int *cus, int *clock_mhz, int *mem_clock_mhz, int *bus_bits);

#ifdef __cplusplus
}
#endif
#endif
