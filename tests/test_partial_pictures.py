"""CPU: partial pictures v1 (csrc/decoder.h) -- the model of tests/partial_model.py against tests/pyhevc.py and the checker where nothing is
lost, the properties the rule promises on a damaged picture, what every stream of tests/partial_cases.py brings, the PRODUCT's host half through the parse-only
hook with the option on (damage log, layout of the missing blocks, unchanged digests where nothing is lost; each probe a child process with a time limit), what
keeping the received rows is worth, and the setter.  The pictures themselves are compared on the GPU (tests/test_gpu_partial_pictures.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conceal_model as cm
import deckit
import enckit
import orc
import parser_probe as PP
import partial_cases as pc
import partial_model as pm
import pyhevc

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. nothing lost
@pytest.mark.parametrize("kw", [dict(seed=3, slices=1, wpp=1, ctb_log2=4, sao=1, tmvp=1), dict(seed=61, slices=3, wpp=1), dict(seed=7, slices=0, wpp=1, gop=4, b_slices=50)])
def test_nothing_lost_the_model_is_pyhevc_and_the_checker(kw):
    g = orc.OracleGen(72, 56, tile_rows=1, tile_cols=1, **kw)
    aus = [g.picture() for _ in range(6)]
    g.close()
    want = deckit.python_pictures(aus)
    od = orc.OracleDecoder()
    ref = [f for t, au in enumerate(aus) for f in od.decode_au(au, t)] + od.flush()
    od.close()
    for mode in (2, 3):
        got, d = pm.decode(aus, deckit.tabs(), mode)
        assert not d.damage and len(got) == len(want) == len(ref)
        assert all(np.array_equal(a["i420"], b["i420"]) and np.array_equal(a["i420"], c["i420"]) for a, b, c in zip(got, want, ref))


# ---- 2. what the rule promises, on the first damaged picture of streams whose reference pictures are intact up to there
def planes_of(pic):
    return enckit.planes(pic["i420"], pic["width"], pic["height"])


def missing_mask(d, w, h, ctb, grow=0):
    """luma mask of the missing coding tree blocks, grown by `grow` samples on every side"""
    m = np.zeros((h, w), bool)
    wc = -(-w // ctb)
    for a, n in d["runs"]:
        for k in range(a, a + n):
            y0, x0 = (k // wc) * ctb, (k % wc) * ctb
            m[max(0, y0 - grow):y0 + ctb + grow, max(0, x0 - grow):x0 + ctb + grow] = True
    return m


@pytest.mark.parametrize("name", ["72x56_ctb16_sao_tmvp", "416x240_ctb64", "pan_refs3"])
def test_properties_of_the_first_damaged_picture(name):
    w, h, aus, _ = pc.stream(name)
    ctb = 1 << (pc.SYNTH[name][3]["ctb_log2"] if name in pc.SYNTH else 6)
    whole = {(p["cvs"], p["poc"]): p for p in deckit.python_pictures(aus)}
    for mode in (2, 3):
        pics, model = pc.model(name, mode)
        d = model.damage[0]
        assert 0 < d["missing"] < d["total"] and d["src_poc"] is not None and not d["src_damaged"]
        got = planes_of(next(p for p in pics if (p["cvs"], p["poc"]) == (d["cvs"], d["poc"])))
        intact, src = planes_of(whole[(d["cvs"], d["poc"])]), planes_of(whole[(d["cvs"], d["src_poc"])])
        far, gone = ~missing_mask(d, w, h, ctb, 8), missing_mask(d, w, h, ctb)
        assert far.any() and gone.any()
        for c in range(3):
            f, g = (far, gone) if c == 0 else (far[::2, ::2], gone[::2, ::2])
            assert np.array_equal(got[c][f], intact[c][f]), "plane %d: a received sample 8 luma samples or more from what is missing differs from the intact decode" % c
            if mode == 2:
                assert np.array_equal(got[c][g], src[c][g]), "plane %d: a missing block is not S's" % c
        if mode == 3:
            moved, disp = cm.stand_in(d["src"], d["poc"])
            assert np.array_equal(disp, d["disp"])
            for c in range(3):
                g = gone if c == 0 else gone[::2, ::2]
                assert np.array_equal(got[c][g], moved[c][g].astype(np.uint8)), "plane %d: a missing block is not conceal_model's stand-in there" % c


# ---- 3. the loss patterns, each asserted to occur: those Kvazaar's row form can have (a lost row takes every later row with it), here; the others -- a first segment lost
# with an independent one behind it, a middle independent one, two gaps in one picture -- on the free-slice streams, below
def test_every_case_has_a_damaged_picture_and_the_patterns_occur():
    seen = set()
    for name in pc.NAMES:
        w, h, aus, arrives = pc.stream(name)
        rows = len(pm.vcl_indices(aus[0]))
        for mode in (2, 3):
            dmg = pc.model(name, mode)[1].damage
            assert any(0 < d["missing"] < d["total"] for d in dmg), name
        wc = dmg[0]["total"] // rows
        for d in dmg:
            assert len(d["runs"]) == 1 and d["runs"][0][0] % wc == 0 and sum(d["runs"][0]) == d["total"]
            seen.add("last segment lost" if d["missing"] == wc else "a middle dependent segment lost that drags the later ones with it")
            seen |= {k for k, v in (("S is itself damaged", d["src_damaged"]), ("a damaged IRAP picture", d["irap"]), ("a damaged B picture", d["b"])) if v}
        if len(arrives) < len(aus):
            seen.add("a whole access unit lost in the same stream")
        if name in pc.SYNTH and any(len(v) == 1 and v[0] < rows - 1 for v in pc.SYNTH[name][4].values()):
            seen.add("segments behind the lost one arrived and were dropped")
    assert seen == {"last segment lost", "a middle dependent segment lost that drags the later ones with it", "S is itself damaged", "a damaged IRAP picture", "a damaged B picture",
                    "a whole access unit lost in the same stream", "segments behind the lost one arrived and were dropped"}, seen


def test_the_free_slice_streams_bring_every_pattern():
    """pictures of free slices without WPP: each pattern of the issue's list occurs, on a damaged picture that has both received and missing blocks"""
    seen = {}
    for name in pc.FREE:
        w, h, aus, arrives = pc.stream(name)
        table = pm.segment_table(aus)
        dmg = pc.model(name, 2)[1].damage
        assert [d["runs"] for d in pc.model(name, 3)[1].damage] == [d["runs"] for d in dmg]
        losses = sorted(pc.free_losses(table).items(), key=lambda kv: kv[1][0])      # (one damaged picture per access unit that lost something, in decoding order)
        assert len(losses) == len(dmg) and len(arrives) == len(aus), name
        for (what, (t, lostk)), d in zip(losses, dmg):
            assert 0 < d["missing"] < d["total"], (name, what)
            if what.startswith("first"):
                assert d["runs"][0][0] == 0 and not table[t][1][1]
            elif what.startswith("two"):
                assert len(d["runs"]) == 2
            elif what.startswith("a middle dependent"):
                assert d["missing"] > table[t][lostk[0] + 1][2] - table[t][lostk[0]][2], "the dependent segment behind the lost one was decoded"
            elif what.startswith("last"):
                assert len(d["runs"]) == 1 and sum(d["runs"][0]) == d["total"]
            seen.setdefault(what, []).append(name)
    assert set(seen) == set(pc.PATTERNS), seen
    assert any(d["b"] for d in pc.model("free_416x240_ctb64_b", 2)[1].damage)


# ---- 4. the product's host half
def child(*args):
    r = subprocess.run([sys.executable, os.path.join(HERE, "partial_cases.py")] + [str(a) for a in args], capture_output=True, timeout=120, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", pc.NAMES + list(pc.FREE))
def test_the_host_half_files_the_models_damage_and_lays_missing_blocks_out_empty(name, threads):
    w, h, _, _ = pc.stream(name)
    dmg = pc.model(name, 2)[1].damage
    r = child(name, threads)
    assert r["log"] == [[d["poc"], a, n] for d in dmg for a, n in d["runs"]]
    assert len(r["layouts"]) == len(dmg)
    for lay, d in zip(r["layouts"], dmg):
        total = len(lay)
        assert total == d["total"]
        wc = -(-w // pc.ctb_of(name))
        hc = total // wc
        assert [a for a in range(total) if lay[a][0]] == [a for f, n in d["runs"] for a in range(f, f + n)]
        for a in range(total):
            missing, byte, nb, blocks = lay[a]
            if not missing:
                continue
            assert blocks == 0, "missing block %d has transform blocks" % a
            k = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    nx, ny = a % wc + dx, a // wc + dy
                    if 0 <= nx < wc and 0 <= ny < hc:
                        q = ny * wc + nx
                        assert not (nb >> k) & 1, "missing block %d is open towards %d" % (a, q)
                        assert not (lay[q][2] >> (7 - k)) & 1, "block %d is open towards the missing block %d" % (q, a)
                        assert lay[q][0] or lay[q][1] != byte, "the received block %d shares the slice byte of the missing block %d" % (q, a)
                    k += 1


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("refs", [1, 3])
def test_the_host_half_on_the_hip_encoders_own_streams(refs, threads):
    """tests/golden/partial/: what arrives of the HIP encoder's slices=wpp streams of tests/test_gpu_partial_pictures_hip_streams.py (320x192, three CTU rows, lp-refs 1
    and 3, row 1's segment of pictures 3 and 4 lost), as written on the GPU: the streams of that GPU table pass the host-half probe too"""
    name = "hip_slices_wpp_refs%d_row1_lost.hevc" % refs
    data = open(os.path.join(HERE, "golden", "partial", name), "rb").read()
    pics, d = pm.decode([data], deckit.tabs(), 2)
    assert len(pics) == 7 and [x["runs"] for x in d.damage] == [[(5, 10)], [(5, 10)]]
    r = child("file:%s:15" % name, threads)
    assert r["log"] == [[x["poc"], 5, 10] for x in d.damage] and len(r["layouts"]) == 2
    for lay in r["layouts"]:
        assert [row[0] for row in lay] == [0] * 5 + [1] * 10 and all(row[3] == 0 and row[1] == 255 for row in lay[5:]) and all(row[1] != 255 for row in lay[:5])
        assert all(not (row[2] >> 6) & 1 for row in lay[:5]), "row 0 is open towards the missing row below"


@pytest.mark.parametrize("name", ["golden_gen_free_slices", "golden_gen_free_slices_wpp", "golden_hip_slices_wpp_qp32", "golden_gen_kvazaar_shaped", "enc_slices_wpp"])
def test_option_on_and_nothing_lost_the_digests_stay(name):
    want = json.load(open(os.path.join(HERE, "golden", "parser_digests.json")))[name]
    for threads in (1, 4):
        r = child("digest:" + name, threads)
        assert (r["digest"], r["pictures"], r["log"]) == (want["digest"], want["pictures"], [])


# ---- 5. what it buys: the checker's encoder with slices=wpp at 640x384 (six CTU rows), row 2's segment of picture 3 lost -- rows 0-1 stay, rows 2-5 are filled
CLIPS = (("pan (3, 1) samples a picture", lambda w, h, n: enckit.pan(w, h, n, 3, 1)), ("benchmark clip", lambda w, h, n: enckit.frames(0, w, h, n)))
W, H, N, LOST, ROW = 640, 384, 7, 3, 2


def behind_the_loss(clip):
    """luma PSNR against the encoder's reconstruction of the damaged picture and the three behind it: [(the whole picture dropped -- pyhevc, v2 --, partial)]"""
    e = enckit.oracle_encoder(W, H, qp=30, subme=2, slices=1)
    aus, recs = [], []
    for f in clip:
        aus.append(e.encode(f))
        recs.append(e.recon())
    e.close()
    part, d = pm.decode([au for _, au in pm.cut(aus, {LOST: (ROW,)})], deckit.tabs(), 2)
    assert len(part) == N and len(d.damage) == 1 and d.damage[0]["runs"] == [(ROW * 10, 40)]
    v2 = pyhevc.Decoder(deckit.tabs())
    shown = None
    for t, au in enumerate(aus):
        if t == LOST:
            continue
        for nal in pyhevc.split_nals(au):
            v2.decode_nal(nal)
        if t == LOST + 1:                                        # what stood in for the dropped picture: the copy v2 made when the next one asked for it
            shown = next(p for p in v2.dpb if p.poc == LOST and getattr(p, "fresh", False))
            shown = np.concatenate([pl.reshape(-1) for pl in shown.planes]).astype(np.uint8)
    drop = {p["poc"]: p["i420"] for p in v2.flush()}
    drop[LOST] = shown
    return [(enckit.psnr_y(drop[t], recs[t], W * H), enckit.psnr_y(part[t]["i420"], recs[t], W * H)) for t in range(LOST, LOST + 4)]


def value_table():
    return {name: behind_the_loss(make(W, H, N)) for name, make in CLIPS}


def table_text(tab):
    lines = ["# partial pictures v1 against dropping the whole picture: luma PSNR (dB) against the encoder's own reconstruction of the damaged picture (number %d of %d; the segment"
             % (LOST, N), "# of CTU row %d of 6 lost, rows 0-%d kept) and of the three pictures behind it; whole picture dropped (tests/pyhevc.py, concealment v2) -> partial" % (ROW, ROW - 1),
             "# (tests/partial_model.py, mode 2); the checker's encoder, slices=wpp, qp 30, subme 2, %dx%d; CPU, deterministic (python tests/test_partial_pictures.py)" % (W, H)]
    for name, rows in tab.items():
        lines.append("%-30s %s" % (name, " / ".join("%.2f -> %.2f" % r for r in rows)))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def table():
    return value_table()


@pytest.mark.parametrize("clip", [c[0] for c in CLIPS])
def test_the_damaged_picture_is_strictly_better_than_a_dropped_one(table, clip):
    """the received rows are exact and the rest is the same copy; nothing is asserted of the pictures behind it"""
    drop, part = table[clip][0]
    print("%s: %.2f -> %.2f dB" % (clip, drop, part))
    assert part > drop


def test_the_value_table_is_the_one_on_record(table):
    """profiles/partial_pictures_cpu.txt (quoted in DESIGN.md section 9.3) is this table"""
    text = table_text(table)
    print(text)
    assert open(os.path.join(os.path.dirname(HERE), "profiles", "partial_pictures_cpu.txt")).read() == text


# ---- 6. the setter
def test_the_setter_is_refused_after_the_first_picture_and_on_a_band_decoder():
    lib = PP._lib()
    lib.kvzx_decoder_set_partial_pictures.argtypes = [C.c_void_p, C.c_int]
    lib.kvzx_decoder_set_band.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.kvzx_decoder_damage.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h = lib.libOpenHevcInit(1, 2)
    try:
        assert lib.kvzx_decoder_set_band(h, 0, 1) == 1 and lib.kvzx_decoder_set_partial_pictures(h, 1) == 0          # a band decoder refuses ...
        assert lib.kvzx_decoder_set_band(h, 0, 0) == 1 and lib.kvzx_decoder_set_partial_pictures(h, 1) == 1 and lib.kvzx_decoder_set_band(h, 0, 1) == 0      # ... and the other way round
        assert lib.kvzx_decoder_set_parse_only(h, 1) == 1 and lib.libOpenHevcStartDecoder(h) == 0
        nals = [n for au in pc.stream("64x64_ctb16_irap")[2][:1] for n in orc.split_nals(au)]
        assert all(lib.libOpenHevcDecode(h, n, len(n), 0) == 0 for n in nals)
        assert lib.kvzx_decoder_set_partial_pictures(h, 0) == 0 and lib.kvzx_decoder_set_partial_pictures(h, 1) == 0           # after the first picture
        missing, total = C.c_int(-1), C.c_int(-1)
        assert lib.kvzx_decoder_damage(h, C.byref(missing), C.byref(total)) == 0                                          # (parse only: no picture was handed out)
    finally:
        lib.libOpenHevcClose(h)


if __name__ == "__main__":
    text = table_text(value_table())
    path = os.path.join(os.path.dirname(HERE), "profiles", "partial_pictures_cpu.txt")
    open(path, "w").write(text)
    print(text)
