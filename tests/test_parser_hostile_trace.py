"""The decoder's host half on hostile input, pinned (CPU, no device): tests/golden/parser_hostile_trace.json holds, for 3000 mutated streams
(parser_probe.mutate, the mutations of tools/fuzz_parser.py), the hash of every libOpenHevcDecode call's return value and kvzx_decoder_last_error and of what
the parser had produced when each trial ended -- recorded before the host half was split into dec_syntax / dec_parse / decoder.  A change to header or assembly
code that returns another code, or returns it from another call, or leaves other state behind for the calls after it, changes the trace."""
import json
import os

import parser_probe as PP

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parser_hostile_trace.json")))


def test_hostile_trace_matches_the_recorded_one():
    got = PP.hostile_trace(GOLDEN["trials"], GOLDEN["threads"])
    assert got["inputs_sha256"] == GOLDEN["inputs_sha256"], \
        "the MUTATED INPUTS differ from the recorded run: the mutation generator or the cases changed (parser_probe.mutate / all_cases), not the decoder"
    assert got["error_calls"] == GOLDEN["error_calls"] and got["trace_sha256"] == GOLDEN["trace_sha256"], \
        "the parser answers broken streams differently: %d calls returned an error (recorded: %d), trace %s (recorded: %s)" % (
            got["error_calls"], GOLDEN["error_calls"], got["trace_sha256"], GOLDEN["trace_sha256"])
