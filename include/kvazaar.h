/*
 * include/kvazaar.h -- C ABI of the MI355X-native HEVC encoder, source-compatible with the part
 * of Kvazaar's public header that uvgComm compiles against.
 *
 * uvgComm reaches its encoder only through this interface
 * (/root/reference/src/media/processing/kvazaarfilter.cpp:8 `#include <kvazaar.h>`):
 *   kvz_api_get(8)                          kvazaarfilter.cpp:145
 *   config_alloc / config_init              kvazaarfilter.cpp:151,160
 *   config_parse(cfg, name, value) == 1 ok  kvazaarfilter.cpp:172-287,363-367
 *   fields written directly                 kvazaarfilter.cpp:223 (target_bitrate), :244 (lossless),
 *                                           :257-276 (mv_constraint), :278 (set_qp_in_cu), :289 (hash)
 *   fields read directly                    kvazaarfilter.cpp:207 (wpp), :299 (owf), :381-384 (width,
 *                                           height, framerate_num, framerate_denom)
 *   encoder_open / encoder_close            kvazaarfilter.cpp:291,317
 *   config_destroy                          kvazaarfilter.cpp:318
 *   picture_alloc / picture_free            kvazaarfilter.cpp:69,54,476
 *   kvz_picture.{y,u,v,pts,roi}             kvazaarfilter.cpp:410-430,53
 *   encoder_encode                          kvazaarfilter.cpp:435-438,445-448
 *   kvz_data_chunk.{data,len,next}          kvazaarfilter.cpp:469-474
 *   chunk_free                              kvazaarfilter.cpp:475
 *
 * The Kvazaar 2.3.1 header itself is not in /root/reference (FetchContent dependency,
 * dependencies/kvazaar.cmake:10-14); the declarations below keep its names and meanings so that
 * kvazaarfilter.cpp compiles unchanged against this file and links against libkvazzup_amd.so
 * (see INTEGRATION.md).  Binary layout compatibility with a Kvazaar-built libkvazaar is NOT
 * claimed: the application must be compiled against this header.
 */
#ifndef KVAZZUP_AMD_KVAZAAR_H_
#define KVAZZUP_AMD_KVAZAAR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define KVZ_PUBLIC __declspec(dllexport)
#else
#define KVZ_PUBLIC __attribute__((visibility("default")))
#endif

#define KVZ_BIT_DEPTH 8
#define KVZ_DATA_CHUNK_SIZE 4096
#define KVZ_MAX_GOP_LENGTH 32

typedef uint8_t kvz_pixel;
typedef struct kvz_encoder kvz_encoder;

enum kvz_chroma_format { KVZ_CSP_400 = 0, KVZ_CSP_420 = 1, KVZ_CSP_422 = 2, KVZ_CSP_444 = 3 };
enum kvz_interlacing { KVZ_INTERLACING_NONE = 0, KVZ_INTERLACING_TFF = 1, KVZ_INTERLACING_BFF = 2 };
enum kvz_mv_constraint {
  KVZ_MV_CONSTRAIN_NONE = 0,
  KVZ_MV_CONSTRAIN_FRAME = 1,
  KVZ_MV_CONSTRAIN_TILE = 2,
  KVZ_MV_CONSTRAIN_FRAME_AND_TILE = 3,
  KVZ_MV_CONSTRAIN_FRAME_AND_TILE_MARGIN = 4
};
enum kvz_hash { KVZ_HASH_NONE = 0, KVZ_HASH_CHECKSUM = 1, KVZ_HASH_MD5 = 2 };
enum kvz_slices { KVZ_SLICES_NONE = 0, KVZ_SLICES_TILES = 1, KVZ_SLICES_WPP = 2 };
enum kvz_sao { KVZ_SAO_OFF = 0, KVZ_SAO_EDGE = 1, KVZ_SAO_BAND = 2, KVZ_SAO_FULL = 3 };
enum kvz_scalinglist { KVZ_SCALING_LIST_OFF = 0, KVZ_SCALING_LIST_CUSTOM = 1, KVZ_SCALING_LIST_DEFAULT = 2 };
enum kvz_rc_algorithm { KVZ_NO_RC = 0, KVZ_LAMBDA = 1, KVZ_OBA = 2 };
enum kvz_ime_algorithm { KVZ_IME_HEXBS = 0, KVZ_IME_TZ = 1, KVZ_IME_FULL = 2, KVZ_IME_FULL8 = 3,
                         KVZ_IME_FULL16 = 4, KVZ_IME_FULL32 = 5, KVZ_IME_FULL64 = 6, KVZ_IME_DIA = 7 };
enum kvz_nal_unit_type { KVZ_NAL_TRAIL_N = 0, KVZ_NAL_TRAIL_R = 1, KVZ_NAL_IDR_W_RADL = 19, KVZ_NAL_IDR_N_LP = 20,
                         KVZ_NAL_CRA_NUT = 21, KVZ_NAL_VPS_NUT = 32, KVZ_NAL_SPS_NUT = 33, KVZ_NAL_PPS_NUT = 34 };
enum kvz_slice_type { KVZ_SLICE_B = 0, KVZ_SLICE_P = 1, KVZ_SLICE_I = 2 };
enum kvz_input_format { KVZ_INPUT_I420 = 0, KVZ_INPUT_RGB32 = 1, KVZ_INPUT_RGB32_SSE41 = 2, KVZ_INPUT_YUYV = 3 };   /* kvz_config.input_format ("input-format", kvazzup_amd extension) */

/* Encoder configuration.  Fields uvgComm touches keep Kvazaar's names; the rest record what
 * config_parse() understood.  Initialise with kvz_api.config_init(). */
typedef struct kvz_config {
  int32_t qp;                 /* "qp" */
  int32_t intra_period;       /* "period": 0 = only first picture, 1 = all intra, n = every n-th */
  int32_t vps_period;         /* "vps-period": parameter sets with every n-th intra picture (0 = first only) */
  int32_t width;              /* "input-res" */
  int32_t height;
  double framerate;           /* deprecated in Kvazaar; kept for source compatibility */
  int32_t framerate_num;      /* "input-fps" */
  int32_t framerate_denom;
  int32_t deblock_enable;     /* "deblock" */
  enum kvz_sao sao_type;      /* "sao": off, or full (edge and band offsets) */
  int32_t rdoq_enable, signhide_enable;   /* "rdoq", "signhide": rate-distortion optimised quantisation ("uvgx RDOQ v1") and sign data hiding in the quantiser (oracle/hevc_enc.c) */
  int32_t smp_enable, amp_enable;         /* recorded; config_parse rejects the value 1 (2NxN / Nx2N / AMP inter partitions are not searched) */
  int32_t rdo;                /* "rd" */
  int32_t full_intra_search, trskip_enable, tr_depth_intra;
  enum kvz_ime_algorithm ime_algorithm;   /* "me": recorded; the GPU search is always exhaustive over +-me_range (a superset of what any of Kvazaar's patterns visits) */
  int32_t fme_level;          /* "subme" (0: integer samples only) */
  int32_t bipred;
  int32_t deblock_beta, deblock_tc;
  int32_t ref_frames;         /* "ref" */
  int32_t tiles_width_count, tiles_height_count;   /* "tiles" CxR: C tile columns x R tile rows, uniform spacing, at most 20 x 22 (a grid finer than the CTU grid is cut down to it) */
  int32_t wpp;                /* "wpp" */
  int32_t owf;                /* "owf": pictures in flight; output is delayed by this many calls */
  int32_t slices;             /* "slices": enum kvz_slices: wpp = a dependent slice segment per CTU row (needs wpp), tiles = an independent slice per tile; one NAL unit each */
  int32_t threads;            /* "threads": host threads of the arithmetic-coding stage (-1 / "auto": 16; 0: the calling thread only) */
  int32_t cpuid;
  int32_t lossless;           /* must be 0 */
  int32_t tmvp_enable;        /* "tmvp": temporal motion vector prediction, collocated picture = the previous picture.  0 (default, also at every preset, unlike Kvazaar): off, the streams of before.  Not in band mode (encoder_open fails) */
  int32_t rdoq_skip, implicit_rdpcm;
  int32_t mv_rdo;
  int32_t calc_psnr;
  enum kvz_mv_constraint mv_constraint;
  enum kvz_hash hash;         /* "hash": decoded picture hash SEI after every picture: none, checksum or md5 (D.3.19), computed from the reconstruction on the device */
  int32_t cu_split_termination, me_early_termination, intra_rdo_et, early_skip;
  int32_t target_bitrate;     /* "bitrate" in bits per second: 0 = constant QP; > 0 = this library's rate control (picture level; with rc_algorithm lambda / oba also between groups of CTU rows, decided on the device) */
  enum kvz_rc_algorithm rc_algorithm;
  int32_t max_merge;
  int32_t gop_len, gop_lowdelay;      /* "gop": lp-g<len>d<depth>t<layers> (and "0") accepted and recorded; without effect unless "lp-gop" is 1 (below) */
  int32_t gop_lp_ref_depth, gop_lp_temporal_layers;   /* d = the number of QP layers (not a reference count: that is "lp-refs"), t = temporal sub-layers (only 1 is implemented) */
  int32_t set_qp_in_cu;
  int32_t vaq;
  enum kvz_scalinglist scaling_list;
  int32_t intra_bits;
  int32_t me_max_steps;
  int32_t fast_residual_cost_limit;
  int32_t pu_depth_inter_min, pu_depth_inter_max, pu_depth_intra_min, pu_depth_intra_max;
  /* kvazzup_amd extensions (not in Kvazaar) */
  int32_t me_range;           /* "me-range": exhaustive search radius in integer samples, 1..32, of the window around the zero vector (and, with "me-coarse", of the second window around the coarse stage's centre: that option is what reaches farther) */
  int32_t gpu_device;         /* "gpu": HIP device ordinal */
  int32_t recon_output;       /* "recon-output": 0 = encoder_encode leaves *pic_out NULL (no download) */
  int32_t intra_satd;         /* "intra-satd": 1 (default) = the intra mode search compares 8x8 Hadamard sums (SATD) like Kvazaar's rough search, 0 = SAD */
  int32_t band_row0, band_rows; /* "band-row0", "band-rows": tile-row split over several encoders (kvazzup_amd.h, kvzx_encoder_band_*); 0 rows = whole picture */
  int32_t input_hold;         /* "input-hold": 1 = the caller leaves a DEVICE input picture (kvzx_encoder_encode_device) unchanged until that picture's access unit has come back, as the kvz_picture contract demands of host pictures; the call then returns without waiting for the input stage (0, default: the buffer may be reused when the call returns) */
  int32_t null_input_poll;    /* "null-input": "drain" (default, Kvazaar's meaning: encoder_encode with pic_in == NULL waits for the oldest picture in flight) or "poll" (it returns a picture only if one has already been finished and never waits: what the loop at kvazaarfilter.cpp:440-448 needs to keep video/OWF pictures in flight instead of emptying the pipeline after every picture) */
  int32_t intra_in_p;         /* "intra-in-p" 0 / 1 / 2: intra coding units in P pictures, 1 = 16x16 units only (presets superfast .. fast), 2 = 16x16 and 8x8 units (medium and slower) ("uvgx intra-in-P v1": a 16x16 quarter whose motion-search cost is high is priced as an intra block from the source picture and coded intra when that is cheaper -- scene cuts, uncovered background); under rate control v2 the row groups are priced without the intra units' levels; ignored in band mode */
  int32_t gpu_entropy;        /* "gpu-entropy": 1 = the arithmetic coder runs on the GPU too (k_cabac_rows: no host coder threads, 2-4 ms more latency per picture), 0 (default) = host thread pool sized by "threads" */
  int32_t intra_chain;        /* "intra-chain" (default 1): the blocks of a CTU whose below-left / above-right reference samples lie in ANOTHER CTU (its left-edge blocks, its above-right corner block) choose among the intra modes that do not read those samples: the CTU wavefront of the reconstruction chain (k_intra_recon, and k_dec_intra on the receiving side) advances in shorter lags; 0 = all 35 modes everywhere */
  int32_t me_source;          /* "me-source" 0 / 1 ("uvgx search pipelining v1"): the integer motion search of a P picture looks at the previous INPUT picture instead of the reference picture's reconstruction, so it depends on nothing the previous picture's reconstruction loop produces and runs beside it on the GPU (fractional refinement, motion compensation and everything behind them use the reconstruction as ever).  On at the presets superfast .. fast, whose subme >= 2 refinement against the reconstruction makes up for it (oracle, 640x384 / 720p: -0.6 .. +0.2 % bits, -0.01 .. -0.02 dB); off at ultrafast (no refinement there: +1.1 .. 1.4 % bits, -0.17 dB) and from medium on; ignored in band mode */
  int32_t lp_refs;            /* "lp-refs" 0..4 (extension, "uvgx multi-reference v1"): with n >= 2 a P picture refers to the min(n, pictures since the last IDR picture) pictures before it, all in list 0 (with "lp-gop" the same count, chosen as that option says).  The gop string says nothing about this count -- its d is the number of QP layers -- so uvgComm users who want three references pass "lp-refs=3" as a custom parameter.  Each 32x32 / 16x16 block searches every reference and codes ref_idx_l0.  0 / 1 (default): one reference, the encoder of before byte for byte ("ref" keeps its meaning and accepts 1 only; "gop" takes effect under "lp-gop" alone).  Not in band mode (encoder_open fails) */
  int32_t me_coarse;          /* "me-coarse" 0 / 64 / 128 / 256 (extension, "uvgx coarse-to-fine search v1"): reach in full samples of a coarse search on quarter-resolution INPUT pictures that gives every 32x32 block and reference a centre; the integer search then looks at its +-me-range window around zero AND, when the centre lies outside it, at a second one around the centre -- vectors of up to me-coarse + me-range samples (scrolling, window drags, pans).  0 (default, also at every preset): the window around zero alone, the encoder of before byte for byte.  Not in band mode (encoder_open fails) */
  int32_t lp_gop;             /* "lp-gop" 0 / 1 (extension, "uvgx low-delay GOP v1"; statement of record: tests/lp_gop_model.py): 1 = gop=lp-g<g>d<d>t1 takes effect -- every g-th picture after an IDR picture is a key picture coded at QP + 1, the pictures between lie on the layers QP + 2 .. QP + d (g4d3: +3, +2, +3, +1), and a P picture refers to the previous picture, the most recent key picture (at most 7 pictures back) and then the pictures before the previous one, "lp-refs" pictures in all; each picture's reference picture set travels in its slice headers, the parameter sets are those of lp-refs.  0 (default, also at every preset), or no gop string / gop=0: the streams of before byte for byte.  encoder_open fails with it in band mode, with t > 1 and with d > 6 */
  int32_t weightp;            /* "weightp" 0 / 1 (extension, "uvgx weighted prediction v1"; restated in tests/wp_model.py): 1 = explicit weighted prediction of luma (PPS weighted_pred_flag, pred_weight_table() in every independent P slice segment header, denominator 6, chroma never weighted).  Per P picture and reference a weight and an offset are derived from the luma mean and variance of the two INPUT pictures and kept when a check on every fourth sample of every fourth row says they pay (16 * weighted SAD < 15 * plain SAD); the integer search then reads weighted copies of its reference planes, and the fractional refinement and the reconstruction predict luma with the weights -- brightness steps, fades, auto-exposure.  0 (default, also at every preset): the streams of before byte for byte.  encoder_open fails with it in band mode and with lossless */
  int32_t intra_refresh;      /* "intra-refresh" 0 / 2..255 (extension, "uvgx intra refresh v1"; restated in tests/ir_model.py): N = the number of P pictures a refresh cycle may take.  A band of intra units (the step ceil(B / N) block columns of 32 samples, B = coded width / 32, plus 16 columns of overlap) walks across the P pictures, one step a picture, cycle after cycle from the first P picture behind an IDR picture; the 32x32 blocks the band has passed keep their vectors out of what it has not.  A decoder that concealed a lost picture has the encoder's pictures again, exactly, once a cycle that began after the loss is complete -- no IDR picture needed, so uvgComm users pass it beside "period=0" or a long period.  The first picture of a cycle carries a recovery point SEI (recovery_poc_cnt = cycle length - 1, exact_match_flag 1).  With "intra-in-p=0" the band's units are the only intra units.  0 (default, also at every preset): the streams of before byte for byte.  encoder_open fails with it beside lp-refs >= 2, lp-gop, tmvp, me-coarse, tiles, band mode, lossless and intra-chain=0 */
  int32_t scenecut;           /* "scenecut" 0 / 1..255 (extension, "uvgx scene cut v1"; restated in tests/scenecut_model.py): N = the least distance in pictures between an IDR picture and a scene-cut IDR picture behind it.  An input picture at least N pictures behind the last IDR picture (and not an IDR picture by "period" anyway) is compared with the previous INPUT picture on their quarter-resolution pictures: the previous one is shifted by the difference of the two means, every visible 8x8 block (32x32 samples) looks for its best match within +-max(8, me-coarse / 4) quarter samples, and a block whose best SAD exceeds its own activity (sum |c - mean|) by more than 128 is new; when more than half of the blocks are new the picture is coded as an IDR picture (POC 0, parameter sets as "vps-period" says) and "period" counts from it -- slide changes, window and camera switches.  Brightness steps, fades and pans within reach are not cuts.  encoder_encode of an examined picture waits for that verdict on the GPU before the picture is planned (DESIGN.md section 9g has the cost); pictures that are not examined wait for nothing.  0 (default, also at every preset): the streams of before byte for byte.  uvgComm users pass it as a custom parameter, e.g. "scenecut=8".  encoder_open fails with it in band mode */
  int32_t input_format;       /* "input-format" i420 / rgb32 / rgb32-sse41 / yuyv (extension; enum kvz_input_format): what the pictures handed to the encoder are.  i420 (default, also at every preset): planar pictures as ever, the encoder of before byte for byte.  Otherwise the encoder takes PACKED pictures through kvzx_encoder_encode_packed_host / _device (kvazzup_amd.h) -- rgb32: width * height * 4 bytes, rows top to bottom, converted with the arithmetic of uvgComm's rgb_to_yuv420_i_c; rgb32-sse41: the same bytes with the arithmetic of rgb_to_yuv420_i_sse41, which turns the picture upside down; yuyv: width * height * 2 bytes Y0 U Y1 V, converted as yuyv_to_yuv420_c does -- and converts them in its input stage on the GPU, in the pass that pads the picture: the stream and the reconstructions are those of an i420 encoder fed the converted pictures, byte for byte.  The format is fixed per encoder; encoder_encode (a kvz_picture carries planes) and the I420 entry points return 0 on such an encoder.  encoder_open fails with it beside input-hold and in band mode, and for rgb32 / rgb32-sse41 when the width is no multiple of 4 */
  int32_t loss_feedback;      /* "loss-feedback" 0 / 1..64 (extension, "uvgx loss feedback v1"; statement of record: tests/fb_model.py): H = how many coded pictures back a loss report may reach -- the encoder keeps that many pictures' motion records on the device.  The application hands the receiver's reports (kvzx_decoder_damage_log's triples) to kvzx_encoder_report_damage (kvazzup_amd.h); the next picture is then a HEAL PICTURE: a P picture that codes as intra units the 16x16 quarters the reported error may have reached along the encoder's own motion since, keeps every other block's vectors out of them, and carries a recovery point SEI (recovery_poc_cnt 0, exact_match_flag 1).  From it on a decoder that handled the loss in any way has the encoder's pictures exactly -- no IDR picture, no parameter sets.  With "intra-in-p=0" the forced quarters are the only intra units.  Without a report no picture changes; 0 (default, also at every preset): the streams of before byte for byte.  encoder_open fails with it beside lp-refs >= 2, lp-gop, tmvp, me-coarse, tiles, band mode, lossless, intra-chain=0 and intra-refresh */
  int32_t fb_anchor;          /* "fb-anchor" 0 / 2..7 (extension, "uvgx loss feedback v2"; statement of record: tests/fb_anchor_model.py): K = how many pictures the encoder and every decoder keep behind the current one.  Beside "loss-feedback" = H >= K.  Every P picture's slice header then lists the K pictures before it (used_by_curr_pic_s0_flag 1 for the previous picture alone), the parameter sets say a picture buffer of K + 1, and the slice data of a picture without a report is that of fb-anchor = 0 bit for bit.  A heal picture whose oldest report names picture n0 is a V2 HEAL PICTURE when the ANCHOR a = n0 - 1 -- the last picture the receiver holds whole -- lies at most K pictures back and not in front of the last IDR or heal picture: it has two references, the previous picture and the anchor; the quarters the error may have reached are searched in the anchor and coded as inter units, where v1 codes them as intra units, so the heal picture is a P picture of roughly ordinary size (reference invalidation).  A report that comes later than that gets v1's heal picture.  kvz_frame_info.ref_list of a v2 heal picture names {t - 1, a}.  0 (default, also at every preset): the streams of before byte for byte.  encoder_open fails with 1, with K > 7, K > H, without loss-feedback, with weightp, where K + 1 exceeds MaxDpbSize of the coded size (1920x1088 and 3840x2176: K <= 5), and with whatever loss-feedback refuses */
} kvz_config;

/* Picture.  y/u/v are planar 8-bit with stride == width (chroma width/2), as uvgComm assumes
 * (kvazaarfilter.cpp:410-418). */
typedef struct kvz_picture {
  kvz_pixel *fulldata_buf;    /* allocation holding all planes */
  kvz_pixel *fulldata;
  kvz_pixel *y, *u, *v;
  kvz_pixel *data[3];
  int32_t width, height, stride;
  struct kvz_picture *base_image;
  int32_t refcount;
  int64_t pts, dts;
  enum kvz_interlacing interlacing;
  enum kvz_chroma_format chroma_format;
  int32_t ref_pocs[16];
  struct {
    int width, height;        /* in 64x64 CTUs */
    int8_t *roi_array;        /* delta QP per CTU, raster; owned by the caller (kvazaarfilter.cpp:426-430,459-463) */
  } roi;
} kvz_picture;

typedef struct kvz_frame_info {
  int32_t poc;
  int8_t qp;
  enum kvz_nal_unit_type nal_unit_type;
  enum kvz_slice_type slice_type;
  int ref_list[2][16];
  int ref_list_len[2];
} kvz_frame_info;

typedef struct kvz_data_chunk {
  uint8_t data[KVZ_DATA_CHUNK_SIZE];
  uint32_t len;
  struct kvz_data_chunk *next;
} kvz_data_chunk;

typedef struct kvz_api {
  kvz_config *(*config_alloc)(void);
  int (*config_destroy)(kvz_config *cfg);
  int (*config_init)(kvz_config *cfg);
  int (*config_parse)(kvz_config *cfg, const char *name, const char *value);   /* 1 = accepted, 0 = rejected */

  kvz_picture *(*picture_alloc)(int32_t width, int32_t height);
  void (*picture_free)(kvz_picture *pic);                                      /* NULL is allowed */

  void (*chunk_free)(kvz_data_chunk *chunk);                                   /* frees the whole list */

  kvz_encoder *(*encoder_open)(const kvz_config *cfg);                         /* NULL on failure */
  void (*encoder_close)(kvz_encoder *encoder);
  int (*encoder_headers)(kvz_encoder *encoder, kvz_data_chunk **data_out, uint32_t *len_out);
  /* Feed one picture (or NULL to flush).  On return *data_out is the access unit of the oldest
   * finished picture (NULL if none), *len_out its size, *pic_out its reconstruction (refcounted,
   * release with picture_free), *src_out the matching source, *info_out its description.
   * Returns 1 on success, 0 on failure. */
  int (*encoder_encode)(kvz_encoder *encoder, kvz_picture *pic_in, kvz_data_chunk **data_out, uint32_t *len_out,
                        kvz_picture **pic_out, kvz_picture **src_out, kvz_frame_info *info_out);
  kvz_picture *(*picture_alloc_csp)(enum kvz_chroma_format chroma_format, int32_t width, int32_t height);
} kvz_api;

/* bit_depth must be 8 (NULL otherwise).  Getting the table does not touch the GPU; encoder_open()
 * returns NULL when no HIP device is usable -- there is no CPU fallback. */
KVZ_PUBLIC const kvz_api *kvz_api_get(int bit_depth);

#ifdef __cplusplus
}
#endif
#endif
