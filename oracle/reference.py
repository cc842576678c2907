"""oracle/reference.py -- what __graft_entry__.build() makes from the reference tree, when that tree is present, into oracle/_ref/ (kept out of
git; nothing of the reference is copied into the repository):

  libyuvconversions_ref.so  the reference's own yuvconversions.cpp, the one source file on the neighbouring path that compiles stand-alone
                            (row f1 of SURVEY.md 8) -- tests/refcolor.py
  compile_checks.json       the drop-in boundary checked by the compiler: the reference's OWN KvazaarFilter /
                            OpenHEVCFilter translation units, compiled where they lie, type-checked against THIS repository's include/ -- and
                            against copies of include/ with one declaration renamed, which must fail -- tests/test_reference_compiles.py

Qt 6 and uvgRTP are absent from the build image, so their few classes the two filter units touch are declared by tests/qtshim/ (test
infrastructure, declarations only); every kvz_api member, kvz_config / kvz_picture / kvz_data_chunk field, enum constant and libOpenHevc*
signature the units use comes from include/."""
import json
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("KVAZZUP_REFERENCE", "/root/reference")
UNITS = ["media/processing/kvazaarfilter.cpp", "media/processing/openhevcfilter.cpp"]
MUTATIONS = [   # (unit, header, needle): with `needle` renamed in a copy of OUR header the unit must no longer compile
    ("media/processing/kvazaarfilter.cpp", "kvazaar.h", "target_bitrate"),               # a kvz_config field uvgComm writes directly (kvazaarfilter.cpp:223)
    ("media/processing/openhevcfilter.cpp", "openHevcWrapper.h", "libOpenHevcGetPictureInfo"),   # openhevcfilter.cpp:199
]
COMPILE_CHECKS = os.path.join(OUT, "compile_checks.json")


def _syntax_only(src, unit, include_dir):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-I", include_dir, "-I", os.path.join(ROOT, "tests", "qtshim"),
           "-I", src, "-I", os.path.join(src, "media", "processing"), "-I", os.path.join(src, "media"), os.path.join(src, unit)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return {"returncode": r.returncode, "stderr": r.stderr}


def compile_checks(src):
    checks = {"units": {}, "mutations": []}
    for unit in UNITS:
        checks["units"][unit] = _syntax_only(src, unit, os.path.join(ROOT, "include"))
    for unit, header, needle in MUTATIONS:
        with tempfile.TemporaryDirectory() as tmp:
            found = False
            for name in os.listdir(os.path.join(ROOT, "include")):
                with open(os.path.join(ROOT, "include", name)) as f:
                    text = f.read()
                if name == header:
                    found = needle in text
                    text = text.replace(needle, needle + "_renamed")
                with open(os.path.join(tmp, name), "w") as f:
                    f.write(text)
            r = _syntax_only(src, unit, tmp)
        checks["mutations"].append(dict(r, unit=unit, header=header, needle=needle, needle_in_header=found))
    return checks


def build(reference=REFERENCE):
    """make oracle/_ref/ from the reference tree; nothing (and True) when the tree is not there"""
    src = os.path.join(reference, "src")
    if not os.path.isdir(src):
        return True
    os.makedirs(OUT, exist_ok=True)
    ok = True
    yuv = os.path.join(src, "media", "processing", "yuvconversions.cpp")
    try:
        subprocess.run(["g++", "-O2", "-mavx2", "-msse4.1", "-fopenmp", "-fPIC", "-shared", "-I", os.path.dirname(yuv), yuv,
                        "-o", os.path.join(OUT, "libyuvconversions_ref.so")], check=True)
    except (OSError, subprocess.CalledProcessError) as e:      # not needed by the hot path; report and go on
        print("oracle/_ref: reference yuvconversions.cpp did not build:", e)
        ok = False
    if shutil.which("g++"):
        with open(COMPILE_CHECKS, "w") as f:
            json.dump(compile_checks(src), f, indent=1)
    return ok


if __name__ == "__main__":
    build()
