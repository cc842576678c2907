"""Generates tests/golden/weightp_intra_refresh_access_units.json from the CPU checker (oracle/hevc_enc.c): the MD5 of every access unit and of every
cropped reconstruction for a few fixed configurations with "weightp" and "intra-refresh" (DESIGN.md sections 9e / 9f), so that a later edit of the
checker cannot move its statement of the two options without the digests saying so (tests/test_oracle_weightp_intra_refresh.py)."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402
import pan_content  # noqa: E402
import wp_model  # noqa: E402

# keyword arguments of orc.OracleEncoder, then the options set by name, in this order; frames: orc.synth_frame(kind, seed, w, h, t), or with "pan" the
# clip pan_content.clip(w, h, frames, vx, vy, seed); "change": wp_model.change() on its luma
CASES = [
    dict(w=320, h=192, kind=0, seed=0x5EED0301, frames=6, change="offset", enc=dict(qp=32, me_range=12, subme=2), opts=(("weightp", 1),)),
    dict(w=320, h=192, kind=0, seed=0x5EED0302, frames=8, change="flash", enc=dict(qp=30, me_range=12, subme=4, sao=1),
         opts=(("lp-refs", 3), ("tmvp", 1), ("weightp", 1), ("intra-in-p", 1))),
    dict(w=200, h=120, kind=0, seed=0x5EED0303, frames=7, change="gain", enc=dict(qp=32, me_range=8, subme=2, bitrate=300000, rc_bands=4),
         opts=(("lp-refs", 3), ("lp-gop-g", 4), ("lp-gop-d", 3), ("lp-gop", 1), ("weightp", 1), ("me-source", 1), ("rdoq", 1), ("signhide", 1))),
    dict(w=320, h=192, kind=0, seed=0x5EED0304, frames=12, change="none", enc=dict(qp=32, me_range=8, subme=2, sao=1), opts=(("intra-refresh", 5), ("intra-in-p", 1))),
    dict(w=320, h=192, kind=0, seed=0x5EED0305, frames=8, pan=[6, 0], change="none", enc=dict(qp=32, me_range=8, subme=4), opts=(("intra-refresh", 5),)),
    dict(w=200, h=120, kind=2, seed=0x5EED0306, frames=10, change="offset", enc=dict(qp=27, me_range=8, subme=2, sao=1, period=6),
         opts=(("intra-refresh", 8), ("weightp", 1), ("intra-in-p", 2), ("hash", 2))),
]


def frames(c):
    if c.get("pan"):
        fr = pan_content.clip(c["w"], c["h"], c["frames"], c["pan"][0], c["pan"][1], c["seed"])
    else:
        fr = [orc.synth_frame(c["kind"], c["seed"], c["w"], c["h"], t) for t in range(c["frames"])]
    return wp_model.change(fr, c["w"], c["h"], c["change"])


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
    return {"w": c["w"], "h": c["h"], "kind": c["kind"], "seed": c["seed"], "frames": c["frames"], "pan": c.get("pan"), "change": c["change"], "enc": c["enc"],
            "opts": [list(o) for o in c["opts"]]}


if __name__ == "__main__":
    doc = {"generator": "tests/golden/make_weightp_intra_refresh_digests.py", "source": "oracle/hevc_enc.c (CPU checker)",
           "cases": [dict(config=case_json(c), frames=digests(c)) for c in CASES]}
    with open(os.path.join(HERE, "weightp_intra_refresh_access_units.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
