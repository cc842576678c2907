"""The decoder's host half alone (include/kvazzup_amd.h kvzx_decoder_set_parse_only): helper shared by tests/test_parser_probe.py and
tests/golden/make_parser_digests.py.  No device is touched; nothing is decoded."""
import ctypes as C
import hashlib
import json
import os
import random

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "streams")
SEED = 0x5EED0000

# streams the checker's encoder writes here: (name, kwargs of OracleEncoder, width, height, pictures, clip kind)
ENCODED = [
    ("enc_plain_320x240_qp32", dict(qp=32, period=64, me_range=16), 320, 240, 5, 0),
    ("enc_noise_qp22", dict(qp=22, period=64, me_range=8), 320, 240, 4, 2),
    ("enc_lowqp_escape_codes", dict(qp=6, period=64, me_range=8), 192, 128, 3, 2),
    ("enc_flat_all_skip", dict(qp=32, period=64, me_range=8), 192, 128, 3, 1),
    ("enc_no_wpp", dict(qp=32, period=4, me_range=16, wpp=0), 416, 240, 5, 0),
    ("enc_tiles_wpp", dict(qp=30, period=3, me_range=16, tile_rows=2), 320, 256, 4, 0),
    ("enc_tiles_2x2_slices", dict(qp=30, period=3, me_range=16, tile_rows=2, tile_cols=2, wpp=0, slices=2), 384, 256, 4, 0),
    ("enc_sao_vaq_subme", dict(qp=30, period=64, me_range=8, sao=1, vaq=8, subme=2), 320, 256, 4, 0),
    ("enc_slices_wpp", dict(qp=32, period=64, me_range=8, slices=1), 320, 256, 3, 0),
    ("enc_720p", dict(qp=32, period=64, me_range=16), 1280, 720, 3, 0),
]


def _lib():
    from kvazzup_amd import _native
    lib = C.CDLL(_native.library_path())
    lib.libOpenHevcInit.restype = C.c_void_p
    lib.libOpenHevcInit.argtypes = [C.c_int, C.c_int]
    for f in (lib.libOpenHevcStartDecoder, lib.libOpenHevcClose, lib.kvzx_decoder_last_error):
        f.argtypes = [C.c_void_p]
    lib.libOpenHevcDecode.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int64]
    lib.kvzx_decoder_set_parse_only.argtypes = [C.c_void_p, C.c_int]
    lib.kvzx_decoder_parse_probe_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    return lib


def probe(nals, threads):
    """parse the NAL units; {'pictures', 'tus', 'levels', 'digest'} of what the parser produced"""
    lib = _lib()
    h = lib.libOpenHevcInit(1, 2)
    assert lib.kvzx_decoder_set_parse_only(h, threads) == 1
    assert lib.libOpenHevcStartDecoder(h) == 0
    try:
        for t, n in enumerate(list(nals) + [bytes([0, 0, 0, 1, 36 << 1, 1])]):      # (end of sequence: a picture of free slices is complete when its access unit has ended)
            rc = lib.libOpenHevcDecode(h, n, len(n), t)
            assert rc == 0, "NAL %d: libOpenHevcDecode returned %d (error %d)" % (t, rc, lib.kvzx_decoder_last_error(h))
        out = (C.c_uint64 * 5)()
        lib.kvzx_decoder_parse_probe_stats(h, out, None)
    finally:
        lib.libOpenHevcClose(h)
    return {"pictures": int(out[0]), "tus": int(out[1]), "levels": int(out[2]), "digest": "%016x" % out[3]}


def golden_cases():
    index = json.load(open(os.path.join(DIR, "index.json")))
    for name in sorted(index):
        yield "golden_" + name, list(orc.split_nals(open(os.path.join(DIR, name + ".hevc"), "rb").read()))


def encoded_case(name):
    for n, kw, w, h, frames, kind in ENCODED:
        if n == name:
            oe = orc.OracleEncoder(w, h, **kw)
            nals = []
            for t in range(frames):
                nals += orc.split_nals(oe.encode(orc.synth_frame(kind, SEED, w, h, t)))
            oe.close()
            return nals
    raise KeyError(name)


def all_cases():
    yield from golden_cases()
    for n, *_ in ENCODED:
        yield n, encoded_case(n)


# ---- hostile input: tools/fuzz_parser.py's mutations, and what the parser ANSWERS to them (tests/test_parser_hostile_trace.py)
def mutate(rng, nals):
    out = [bytearray(n) for n in nals]
    for _ in range(rng.choice((1, 1, 1, 2, 3, 6))):
        kind = rng.random()
        i = rng.randrange(len(out))
        n = out[i]
        hdr = 6                                                    # start code + NAL header
        if kind < 0.35 and len(n) > hdr:                           # bit flips, anywhere behind the NAL header (the first bytes twice as often)
            for _ in range(rng.choice((1, 1, 2, 4, 16))):
                p = rng.randrange(hdr, len(n)) if rng.random() < 0.5 else rng.randrange(hdr, min(len(n), hdr + 24))
                n[p] ^= 1 << rng.randrange(8)
        elif kind < 0.5 and len(n) > hdr + 1:                      # a run overwritten
            p = rng.randrange(hdr, len(n)); k = min(len(n) - p, rng.choice((1, 2, 4, 8, 64)))
            n[p:p + k] = bytes(rng.randrange(256) for _ in range(k)) if rng.random() < 0.7 else bytes([rng.choice((0, 0xff))]) * k
        elif kind < 0.65 and len(n) > hdr + 1:                     # truncation
            del n[rng.randrange(hdr, len(n)):]
        elif kind < 0.72:                                          # insertion
            p = rng.randrange(hdr, len(n) + 1); n[p:p] = bytes(rng.randrange(256) for _ in range(rng.choice((1, 2, 3, 8))))
        elif kind < 0.8 and len(out) > 1:                          # a NAL unit dropped
            del out[i]
        elif kind < 0.87:                                          # ... duplicated
            out.insert(i, bytearray(n))
        elif kind < 0.94 and len(out) > 1:                         # ... swapped with another
            j = rng.randrange(len(out)); out[i], out[j] = out[j], out[i]
        elif kind < 0.97:                                          # the NAL header itself (type, layer, temporal id)
            if len(n) > 5:
                n[4 + rng.randrange(2)] = rng.randrange(256)
        elif len(n) > hdr + 2:                                     # a run of zero BITS spliced into the head (parameter sets, slice headers): an Exp-Golomb field of any size, wherever it lands
            head = min(len(n), hdr + 40)
            bits = "".join("{:08b}".format(b) for b in n[hdr:head])
            at = rng.randrange(len(bits))
            bits = bits[:at] + "0" * rng.choice((8, 16, 24, 30, 31, 32, 33, 48)) + "1" + bits[at:]
            bits += "0" * (-len(bits) % 8)
            n[hdr:head] = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return [bytes(n) for n in out if len(n) > 4]


def hostile_trace(trials, threads=1, first_seed=1):
    """trials first_seed .. first_seed + trials - 1 as tools/fuzz_parser.py draws them (case, its thread choice -- drawn and dropped: `threads` holds --, mutation):
    SHA-256 of the mutated inputs; SHA-256 of every call's (libOpenHevcDecode return value, kvzx_decoder_last_error) and the trial's first four probe statistics;
    the count of calls that returned an error code.  The trace depends on the parse thread count (pictures of a broken stream fail at different rows): compare like with like."""
    cases = list(all_cases())
    lib = _lib()
    h_in, h_out, errors = hashlib.sha256(), hashlib.sha256(), 0
    for seed in range(first_seed, first_seed + trials):
        rng = random.Random(seed)
        name, nals = cases[rng.randrange(len(cases))]
        rng.choice(["1", "4"])
        mut = mutate(rng, nals)
        h_in.update(repr((seed, name, mut)).encode())
        d = lib.libOpenHevcInit(1, 2)
        assert lib.kvzx_decoder_set_parse_only(d, threads) == 1 and lib.libOpenHevcStartDecoder(d) == 0
        calls = []
        for k, n in enumerate(mut):
            rc = lib.libOpenHevcDecode(d, n, len(n), k)
            calls.append((rc, lib.kvzx_decoder_last_error(d)))
            errors += rc < 0
        out = (C.c_uint64 * 5)()
        lib.kvzx_decoder_parse_probe_stats(d, out, None)
        lib.libOpenHevcClose(d)
        h_out.update(repr((seed, calls, list(out)[:4])).encode())
    return {"trials": trials, "threads": threads, "inputs_sha256": h_in.hexdigest(), "trace_sha256": h_out.hexdigest(), "error_calls": int(errors)}
