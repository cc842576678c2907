"""CPU: the streams of tests/test_gpu_batch_foreign.py (tests/batch_cases.py) bring what they are there for -- from the synthesiser's returned configuration, the
checker's decoder, tests/pyhevc.py and the model decoder alone."""
import batch_cases as bc
import cases


def general(config):
    """what DecFrame::general says of the stream's pictures: more than one slice, a tile grid, or PCM"""
    return config is not None and (config["slices"] > 0 or config["tile_rows"] > 1 or config["tile_cols"] > 1 or config["pcm"] > 0)


def test_the_eight_forms():
    streams = bc.eight_forms()
    assert len(streams) == 8 and [s["threads"] for s in streams] == [1, 4] * 4
    for (w, h, _), s in zip(bc.FORMS, streams):
        assert (s["w"], s["h"]) == (w, h) and len(s["aus"]) == len(s["want"]) == 8
        assert all((f["width"], f["height"]) == (w, h) for f in s["want"])
    cfg = [s["config"] for s in streams]
    assert any(general(c) for c in cfg) and any(not general(c) for c in cfg)
    assert general(cfg[bc.TILES]) and general(cfg[bc.PCM]) and not general(cfg[bc.TINY]) and not general(cfg[bc.LONG_TERM]) and cfg[bc.KVAZAAR] is None
    ctb = {c["ctb_log2"] for c in cfg if c}
    assert ctb == {4, 5, 6}                                    # (the checker's encoder: 64 samples as well)
    assert cfg[bc.TILES]["lf_across"] == 2 and cfg[bc.PCM]["slices"] == 3 and cfg[bc.PCM]["lf_across"] == 1
    assert cfg[bc.CTB16]["min_cb_log2"] == 3                   # (200x136 is no multiple of 16: the synthesiser keeps 8; minimum coding blocks of 16 and 32 come with the draws of (d))
    assert [k for k, c in enumerate(cfg) if c and c["b_slices"] > 0] == [bc.B_SLICES]
    b = cfg[bc.B_SLICES]
    assert b["gop"] == 4 and b["weighted"] == 50 and b["list_mod"] == 50 and b["num_refs"] == 2
    assert cfg[bc.SCALING]["scaling_lists"] == 4 and cfg[bc.SCALING]["tq_bypass"] == 20 and cfg[bc.LONG_TERM]["long_term"] == 1
    pts = [f["pts"] for f in streams[bc.B_SLICES]["want"]]
    assert sorted(pts) == list(range(8)) and pts != sorted(pts)          # (the pictures leave in another order than they arrive)


def test_ten_decoders_are_the_eight_and_two_more():
    streams = bc.ten_decoders()
    assert len(streams) == 10 and [(s["w"], s["h"]) for s in streams[8:]] == [(24, 16), (64, 64)]
    assert streams[8]["config"]["seed"] == streams[9]["config"]["seed"] == bc.SEED + 1
    assert streams[8]["aus"] != streams[bc.TINY]["aus"] and streams[9]["aus"] != streams[bc.LONG_TERM]["aus"]
    assert bc.total(streams) == 80


def test_the_cip_stream_takes_both_paths():
    streams = bc.cip_hop()
    s = streams[0]
    print(" ".join(s["kinds"]))
    assert s["config"]["cip"] == 1 and len(s["kinds"]) == 12
    assert 2 <= s["mixed"] <= 10
    hops = sum(1 for a, b in zip(s["kinds"], s["kinds"][1:]) if (a == "IP") != (b == "IP"))
    assert hops >= 2                                           # to its own launches and back
    assert [len(x["want"]) for x in streams] == [12, 12, 12] and [x["threads"] for x in streams] == [1, 4, 1]
    for k, whole in ((1, bc.form(bc.CTB16)), (2, bc.form(bc.TINY))):          # the streams of (a), four pictures longer
        assert streams[k]["aus"][:8] == whole["aus"]


def test_the_lossy_streams_conceal():
    streams = bc.lost_pictures()
    assert [s["threads"] for s in streams] == [3, 1, 1, 1] and [s.get("concealment") for s in streams] == [None, None, 3, None]
    for s in streams[:3]:
        assert s["lost"] > 0 and len(s["aus"]) == 26 - s["lost"] == len(s["want"])
    assert streams[0]["concealed"] > 0 and streams[1]["concealed"] > 0
    assert streams[2]["moved"] >= 1
    print("mode 3: seed %d, %d stand-ins moved" % (bc.mode3_seed(), streams[2]["moved"]))
    assert len(streams[3]["want"]) == 24 and [f["pts"] for f in streams[3]["want"]] == list(range(24))
    assert streams[3]["aus"][:8] == bc.form(bc.KVAZAAR)["aus"]


def test_the_peer_that_is_alone_is_all_intra():
    a, b, c = bc.join_and_leave()
    assert a["config"]["intra_period"] == 1 and a["config"]["nxn_intra"] == 1 and a["threads"] == 4 and len(a["want"]) == 12 and (a["w"], a["h"]) == (352, 288)
    assert b["start_after"] == (0, 3) and c["start_after"] == (0, 8) and b["close_early"] and c["close_early"] and not a.get("start_after")
    assert b["aus"] == bc.form(bc.LONG_TERM)["aus"] and c["aus"] == bc.form(bc.TINY)["aus"]


def test_the_draws_are_those_of_everything_at_once():
    """(the streams themselves are made by the GPU test: 48 of them, seconds)"""
    plan = [row for group in range(12) for row in bc.everything_plan(group)]
    assert [row[0] for row in plan] == list(range(1, 49))
    for seed, w, h, kw, n, threads in plan:
        assert (w, h, kw) == cases.drawn(seed) and n == (12 if kw.get("long_term") else 6) and threads == (3 if seed & 1 else 1)
    s = bc.everything(7)[0]                                    # one of them built: the options arrive in the generator
    seed, w, h, kw, n, threads = bc.everything_plan(7)[0]
    assert s["config"]["seed"] == seed and all(s["config"][k] == v for k, v in kw.items()) and len(s["want"]) == n and s["threads"] == threads
