#!/usr/bin/env python3
"""tests/golden/make_hostile_trace.py -- what the PRODUCT's host half ANSWERS to broken streams: trials seed = 1 .. 3000 of tools/fuzz_parser.py's mutations
(parser_probe.mutate) over parser_probe.all_cases(), one parse thread; SHA-256 of the mutated inputs, SHA-256 of every call's (libOpenHevcDecode return value,
kvzx_decoder_last_error) plus each trial's first four probe statistics, and the count of calls that returned an error code.  tests/parser_digests.json pins what
the parser produces for valid streams; this pins which call returns which code for a broken one.  Recorded with the library before the decoder's host half was
split into dec_syntax / dec_parse / decoder; tests/test_parser_hostile_trace.py (CPU) holds every later one to it.

  KVAZZUP_AMD_LIBRARY=<that library> python tests/golden/make_hostile_trace.py > tests/golden/parser_hostile_trace.json
  ... --trials 20000 --threads 4        # a wider comparison of two libraries (the trace differs BETWEEN thread counts: compare like with like)"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import parser_probe as PP                                                    # noqa: E402

TRIALS = 3000

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=TRIALS)
    ap.add_argument("--threads", type=int, default=1)
    a = ap.parse_args()
    json.dump(PP.hostile_trace(a.trials, a.threads), sys.stdout, indent=1, sort_keys=True)
    print()
