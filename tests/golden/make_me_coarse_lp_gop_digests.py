"""Generates tests/golden/me_coarse_lp_gop_access_units.json from the CPU checker (oracle/hevc_enc.c): the MD5 of every access unit and of every
cropped reconstruction for a few fixed configurations with "me-coarse" and "lp-gop" (DESIGN.md sections 9c / 9d), so that a later edit of the
checker cannot move its statement of the two features without the digests saying so (tests/test_oracle_me_coarse_lp_gop.py)."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402
import pan_content  # noqa: E402

# keyword arguments of orc.OracleEncoder, then the options set by name, in this order; frames: orc.synth_frame(kind, seed, w, h, t), or with "pan" the
# clip pan_content.clip(w, h, frames, vx, vy, seed)
CASES = [
    dict(w=256, h=128, kind=0, seed=0x5EED0201, frames=4, pan=[44, -36], enc=dict(qp=32, me_range=8), opts=(("me-coarse", 64),)),
    dict(w=384, h=256, kind=0, seed=0x5EED0202, frames=5, pan=[-72, 40], enc=dict(qp=30, me_range=16, subme=4, sao=1),
         opts=(("lp-refs", 3), ("tmvp", 1), ("me-coarse", 128), ("intra-in-p", 1))),
    dict(w=320, h=192, kind=0, seed=0x5EED0203, frames=8, pan=[150, 9], enc=dict(qp=32, me_range=12, subme=2, tile_rows=2, tile_cols=2, wpp=0, mv_frame=2),
         opts=(("me-coarse", 256), ("me-source", 1))),
    dict(w=320, h=192, kind=0, seed=0x5EED0204, frames=10, enc=dict(qp=32, me_range=12), opts=(("lp-refs", 3), ("lp-gop-g", 4), ("lp-gop-d", 3), ("lp-gop", 1))),
    dict(w=320, h=192, kind=2, seed=0x5EED0205, frames=12, enc=dict(qp=49, me_range=8, me_early=0, subme=2, period=7),
         opts=(("lp-refs", 4), ("tmvp", 1), ("lp-gop-g", 8), ("lp-gop-d", 4), ("lp-gop", 1), ("intra-in-p", 2))),
    dict(w=320, h=192, kind=0, seed=0x5EED0206, frames=12, enc=dict(qp=32, me_range=12, bitrate=300000, rc_bands=4, sao=1),
         opts=(("lp-refs", 3), ("tmvp", 1), ("lp-gop-g", 4), ("lp-gop-d", 3), ("lp-gop", 1), ("hash", 2))),
    dict(w=130, h=70, kind=0, seed=0x5EED0207, frames=8, pan=[36, -40], enc=dict(qp=30, me_range=8, subme=4, vaq=6),
         opts=(("lp-refs", 3), ("tmvp", 1), ("lp-gop-g", 3), ("lp-gop-d", 2), ("lp-gop", 1), ("me-coarse", 64), ("me-source", 1))),
]


def frames(c):
    if c.get("pan"):
        return pan_content.clip(c["w"], c["h"], c["frames"], c["pan"][0], c["pan"][1], c["seed"])
    return [orc.synth_frame(c["kind"], c["seed"], c["w"], c["h"], t) for t in range(c["frames"])]


def digests(c):
    e = orc.OracleEncoder(c["w"], c["h"], **c["enc"])
    for name, value in c["opts"]:
        e.set_option(name, value)
    out = []
    for fr in frames(c):
        au = e.encode(fr)
        out.append({"au_bytes": len(au), "au_md5": hashlib.md5(au).hexdigest(), "recon_md5": hashlib.md5(e.recon().tobytes()).hexdigest()})
    e.close()
    return out


def case_json(c):
    return {"w": c["w"], "h": c["h"], "kind": c["kind"], "seed": c["seed"], "frames": c["frames"], "pan": c.get("pan"), "enc": c["enc"],
            "opts": [list(o) for o in c["opts"]]}


if __name__ == "__main__":
    doc = {"generator": "tests/golden/make_me_coarse_lp_gop_digests.py", "source": "oracle/hevc_enc.c (CPU checker)",
           "cases": [dict(config=case_json(c), frames=digests(c)) for c in CASES]}
    with open(os.path.join(HERE, "me_coarse_lp_gop_access_units.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
