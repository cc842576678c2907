"""The drop-in boundary, checked by the compiler: the reference's OWN KvazaarFilter / OpenHEVCFilter translation
units -- media/processing/kvazaarfilter.cpp and openhevcfilter.cpp of the reference tree, compiled where they lie, nothing copied -- type-check
against THIS repository's include/kvazaar.h and include/openHevcWrapper.h.  Qt 6 and uvgRTP are absent from the build image, so their few
classes the two files touch are declared by tests/qtshim/ (test infrastructure, declarations only); every kvz_api member, kvz_config /
kvz_picture / kvz_data_chunk field, enum constant and libOpenHevc* signature the files use comes from include/.

The compiles run in build() (oracle/reference.py), which records their outcomes in oracle/_ref/compile_checks.json; these tests read that
record.  Skipped where build() had no reference tree to compile from (the GPU box)."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = os.path.join(ROOT, "oracle", "_ref", "compile_checks.json")
UNITS = ["media/processing/kvazaarfilter.cpp", "media/processing/openhevcfilter.cpp"]

pytestmark = pytest.mark.skipif(not os.path.exists(CHECKS), reason="oracle/_ref not built (needs the reference tree at build time)")


def _checks():
    with open(CHECKS) as f:
        return json.load(f)


@pytest.mark.parametrize("unit", UNITS)
def test_reference_filter_compiles_against_our_headers(unit):
    r = _checks()["units"][unit]
    assert r["returncode"] == 0, r["stderr"]


@pytest.mark.parametrize("unit,header,needle", [
    ("media/processing/kvazaarfilter.cpp", "kvazaar.h", "target_bitrate"),            # a kvz_config field uvgComm writes directly (kvazaarfilter.cpp:223)
    ("media/processing/openhevcfilter.cpp", "openHevcWrapper.h", "libOpenHevcGetPictureInfo"),   # openhevcfilter.cpp:199
])
def test_the_check_notices_a_missing_declaration(unit, header, needle):
    """the compile test is a real check: with the named field / function renamed in a scratch copy of OUR header the reference's file no longer compiles"""
    r = [m for m in _checks()["mutations"] if (m["unit"], m["header"], m["needle"]) == (unit, header, needle)]
    assert len(r) == 1, "build() recorded no compile with %s renamed in %s" % (needle, header)
    r = r[0]
    assert r["needle_in_header"]
    assert r["returncode"] != 0 and needle in r["stderr"], r["stderr"][-2000:]
