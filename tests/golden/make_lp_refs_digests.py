"""Generates tests/golden/lp_refs_tmvp_access_units.json from the CPU checker (oracle/hevc_enc.c): the MD5 of every access unit and of every
cropped reconstruction for a few fixed configurations with "lp-refs" 2..4 and "tmvp" (DESIGN.md sections 9a / 9b), so that a later edit of the
checker cannot move its statement of the two features without the digests saying so (tests/test_oracle_lp_refs_tmvp.py)."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402

# keyword arguments of orc.OracleEncoder, then the options set by name; frames of orc.synth_frame(kind, seed, w, h, t)
CASES = [
    dict(w=256, h=128, kind=0, seed=0x5EED0101, frames=6, enc=dict(qp=32, me_range=8), opts=(("lp-refs", 2),)),
    dict(w=320, h=192, kind=0, seed=0x5EED0102, frames=7, enc=dict(qp=30, me_range=12, subme=4), opts=(("lp-refs", 3), ("tmvp", 1))),
    dict(w=320, h=192, kind=2, seed=0x5EED0103, frames=6, enc=dict(qp=27, me_range=8, me_early=0), opts=(("lp-refs", 4), ("tmvp", 1), ("intra-in-p", 2))),
    dict(w=448, h=320, kind=0, seed=0x5EED0104, frames=6, enc=dict(qp=32, me_range=8, tile_rows=2, tile_cols=2, slices=2, sao=1, period=4),
         opts=(("lp-refs", 3), ("tmvp", 1))),
    dict(w=320, h=192, kind=0, seed=0x5EED0105, frames=9, enc=dict(qp=32, me_range=12, bitrate=300000, rc_bands=4, subme=2),
         opts=(("lp-refs", 4), ("tmvp", 1), ("me-source", 1), ("intra-in-p", 1))),
    dict(w=130, h=70, kind=0, seed=0x5EED0106, frames=6, enc=dict(qp=30, me_range=8, period=5), opts=(("lp-refs", 2), ("tmvp", 1), ("hash", 2))),
]


def digests(c):
    e = orc.OracleEncoder(c["w"], c["h"], **c["enc"])
    for name, value in c["opts"]:
        e.set_option(name, value)
    out = []
    for t in range(c["frames"]):
        au = e.encode(orc.synth_frame(c["kind"], c["seed"], c["w"], c["h"], t))
        out.append({"au_bytes": len(au), "au_md5": hashlib.md5(au).hexdigest(), "recon_md5": hashlib.md5(e.recon().tobytes()).hexdigest()})
    e.close()
    return out


def case_json(c):
    return {"w": c["w"], "h": c["h"], "kind": c["kind"], "seed": c["seed"], "frames": c["frames"], "enc": c["enc"], "opts": [list(o) for o in c["opts"]]}


if __name__ == "__main__":
    doc = {"generator": "tests/golden/make_lp_refs_digests.py", "source": "oracle/hevc_enc.c (CPU checker)",
           "cases": [dict(config=case_json(c), frames=digests(c)) for c in CASES]}
    with open(os.path.join(HERE, "lp_refs_tmvp_access_units.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
