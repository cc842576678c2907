"""CPU: the decoder's output-order rules (kvazzup_amd/csrc/dec_order.h through tests/hostcheck/order.cpp, payload = the picture's serial) against a restatement of
C.5.2 as tests/pyhevc.py states it (Decoder.bump / flush, the CVS start in decode_slice, picture_done).

Inputs are shaped like the synthesiser's streams: coded video sequences of hierarchical groups of 1, 2, 4 or 8 pictures with the reorder count oracle/hevc_gen.c
writes for the group size, IRAP pictures that start them (some with no_output_of_prior_pics_flag in force), pictures with pic_output_flag = 0, end of sequence NAL
units between some sequences.  The rules are driven the way Decoder::decode_nal drives them under frame threads: per call one picture is submitted, the picture
`lag` positions back completes (unless it is never output), and at most one picture is handed out."""
import collections
import ctypes as C
import random

import pytest

import hc

SEEDS = (1, 2, 3, 4, 5, 6)
LAGS = (0, 1, 3, 8)
EOS = "eos"


def group_order(g):
    """oracle/hevc_gen.c gop_order: the last picture of the group, then the middle of every interval, depth first"""
    order, stack = [g], [(0, g)]
    while stack:
        a, b = stack.pop()
        m = (a + b) // 2
        if m == a:
            continue
        order.append(m)
        stack += [(m, b), (a, m)]
    return order


def make_stream(seed):
    """-> [picture dict | EOS]: poc, reorder, starts_cvs, discard_prior, shown, in decoding order"""
    rng = random.Random(seed)
    items, after_eos = [], True
    for s in range(14):
        g = rng.choice((1, 2, 4, 8))
        reorder = g.bit_length() - 1
        discard = bool(items) and not after_eos and rng.random() < 0.5      # (never in force on the first picture or behind an end of sequence: Decoder::slice_front)
        items.append(dict(poc=0, reorder=reorder, starts_cvs=True, discard_prior=discard, shown=True, in_group=False))
        for k in range(rng.randrange(1, 4)):
            for off in group_order(g):
                items.append(dict(poc=k * g + off, reorder=reorder, starts_cvs=False, discard_prior=False, shown=rng.random() >= 0.12, in_group=g > 1))
        after_eos = rng.random() < 0.35
        if after_eos:
            items.append(EOS)
    return items


class Model:
    """C.5.2 as tests/pyhevc.py applies it; pictures are named by their index in the stream"""

    def __init__(self):
        self.waiting, self.out, self.dropped = [], [], []

    def bump(self):
        k = min(range(len(self.waiting)), key=lambda i: self.waiting[i][1])
        self.out.append(self.waiting.pop(k)[0])

    def flush(self):
        while self.waiting:
            self.bump()

    def picture(self, i, p):
        if p["starts_cvs"]:
            if p["discard_prior"]:
                self.dropped += [w[0] for w in self.waiting]
                self.waiting = []
            self.flush()
        else:
            while len(self.waiting) > p["reorder"]:
                self.bump()
        if p["shown"]:
            self.waiting.append((i, p["poc"]))
            while len(self.waiting) > p["reorder"]:
                self.bump()


def run_model(items, lag):
    """-> (output order, what the stream covers at this lag, the pictures discarded)"""
    m, seen = Model(), set()
    for i, p in enumerate(items):
        if p == EOS:
            if m.waiting:
                seen.add("eos_flush_with_pictures_waiting")
            m.flush()
            continue
        if p["starts_cvs"] and m.waiting:
            if p["discard_prior"]:
                done = sum(1 for q in items[:i] if q != EOS)      # pictures submitted before this one; the first done - lag of them have completed
                pos = {j: sum(1 for q in items[:j] if q != EOS) for j, _ in m.waiting}
                seen |= {"discard_hits_completed" if pos[j] < done - lag else "discard_hits_not_completed" for j, _ in m.waiting}
            elif p["reorder"] == 0:
                seen.add("plain_sequence_behind_waiting_pictures")
        if not p["shown"] and p["in_group"]:
            seen.add("no_output_in_group")
        m.picture(i, p)
    m.flush()
    return m.out, seen, m.dropped


def run_rules(items, lag, seed, ahead):
    """Decoder::decode_nal's use of the rules -> the indices in the order they were handed out, the indices whose payloads came back for release, how often a picture
    completed ahead of its turn {"plain_behind_queued", "plain", "reordering"}"""
    L, rng = hc.lib(), random.Random(seed * 1000 + lag)
    h = L.ho_new()
    out, back, pending, index_of, cvs, ahead_seen = [], [], [], {}, 0, collections.Counter()
    dropped, nd, got = (C.c_uint64 * 64)(), C.c_int(), C.c_uint64()

    def call(done, flush, in_turn=True):
        """one decode call: `done` (or None) completes in it"""
        ready = done is not None and done["shown"] and not L.ho_discarded(h, done["serial"])
        if in_turn and L.ho_idle(h) and not (ready and done["reorder"] > 0):
            if ready:
                out.append(index_of[done["serial"]])                  # the fast path: handed out where it lies
            return
        if ready and not in_turn:
            ahead_seen["reordering" if done["reorder"] > 0 else "plain" if L.ho_idle(h) else "plain_behind_queued"] += 1
        if ready:
            L.ho_completed(h, done["serial"], done["poc"], done["cvs"], done["reorder"], int(in_turn))
        if in_turn and L.ho_next(h, int(flush), C.byref(got)):
            out.append(index_of[got.value])

    try:
        for i, p in enumerate(items):
            if p == EOS:
                L.ho_sequence_ended(h)
                call(pending.pop(0) if pending else None, flush=not pending)      # (flush: nothing is left in the pipeline after this call's picture)
                continue
            p = dict(p)
            cvs += p["starts_cvs"]
            p["cvs"] = cvs
            args = (p["poc"], p["reorder"], int(p["starts_cvs"]), int(p["discard_prior"]), int(not p["shown"]), dropped, 64, C.byref(nd))
            if not p["starts_cvs"] and rng.random() < 0.1:                # a picture taken back and submitted again (Decoder::take_back_job)
                L.ho_mark(h)
                L.ho_submitted(h, *args)
                L.ho_restore(h)
            p["serial"] = L.ho_submitted(h, *args)
            back += [index_of[dropped[k]] for k in range(nd.value)]
            index_of[p["serial"]] = i
            pending.append(p)
            if ahead and len(pending) > lag and rng.random() < 0.2:   # a picture completed ahead of its turn, the call then completes none in turn
                call(pending.pop(0), False, in_turn=False)
            call(pending.pop(0) if len(pending) > lag else None, False)
        while pending:
            call(pending.pop(0), flush=not pending)
        while L.ho_next(h, 1, C.byref(got)):
            out.append(index_of[got.value])
        assert L.ho_idle(h)
    finally:
        L.ho_free(h)
    return out, back, ahead_seen


@pytest.mark.parametrize("ahead", (False, True))
@pytest.mark.parametrize("lag", LAGS)
def test_pictures_leave_in_the_order_of_c_5_2(lag, ahead):
    ahead_seen = collections.Counter()
    for seed in SEEDS:
        items = make_stream(seed)
        want, _, discarded = run_model(items, lag)
        got, back, seen = run_rules(items, lag, seed, ahead)
        ahead_seen += seen
        assert got == want, (seed, lag, ahead)
        assert set(back) <= set(discarded) and len(set(back)) == len(back), (seed, lag, ahead)
        assert lag > 0 or sorted(back) == sorted(discarded), (seed, ahead)      # (nothing in the pipeline: every discarded picture had completed and comes back)
    assert all(ahead_seen[k] > 0 for k in ("plain_behind_queued", "reordering")) if ahead else not ahead_seen, ahead_seen


def test_the_streams_cover_what_they_are_for():
    seen = set()
    for seed in SEEDS:
        for lag in LAGS:
            seen |= run_model(make_stream(seed), lag)[1]
    assert seen == {"plain_sequence_behind_waiting_pictures", "discard_hits_not_completed", "discard_hits_completed", "no_output_in_group", "eos_flush_with_pictures_waiting"}


def calls(*sequences):
    """lag 0, nothing in the pipeline: sequences of (pictures as (POC, starts a sequence), reorder count), every picture completing in the call that submits it
    -> per call the serial handed out, or None"""
    L = hc.lib()
    h = L.ho_new()
    dropped, nd, got, log = (C.c_uint64 * 4)(), C.c_int(), C.c_uint64(), []
    try:
        for cvs, (pics, nr) in enumerate(sequences, 1):
            for poc, starts in pics:
                s = L.ho_submitted(h, poc, nr, int(starts), 0, 0, dropped, 4, C.byref(nd))
                if L.ho_idle(h) and nr == 0:
                    log.append(s)                                     # the fast path
                    continue
                L.ho_completed(h, s, poc, cvs, nr, 1)
                log.append(got.value if L.ho_next(h, 0, C.byref(got)) else None)
    finally:
        L.ho_free(h)
    return log


@pytest.mark.parametrize("g2", (1, 4))
def test_what_waited_for_an_old_sequence_leaves_one_picture_per_call(g2):
    """The call in which pictures leave: a sequence of groups of four (two pictures may overtake one) and a new sequence behind it that does not reorder (g2 = 1)
    or does (g2 = 4).  The old sequence ends with two pictures waiting.  From the call that completes the new sequence's first picture every call hands out exactly
    one picture -- the two that waited first, in POC order -- and a sequence that does not reorder keeps that lag of two to its end."""
    old = [(0, True)] + [(off, False) for off in group_order(4)]
    new = [(0, True)] + [(k * g2 + off, False) for k in range(3) for off in group_order(g2)]
    log = calls((old, 2), (new, g2.bit_length() - 1))
    assert log[:5] == [None, None, 1, 4, 3]                           # decoded as POC 0, 4, 2, 1, 3: POC 0 leaves once three wait, then 1, then 2; 3 (serial 5) and 4 (serial 2) still wait
    assert log[5:7] == [5, 2]                                         # the new sequence's first two calls: what waited, by POC
    assert None not in log[5:] and len(set(log[5:])) == len(log[5:])
    if g2 == 1:
        assert log[7:] == list(range(6, 6 + len(new) - 2))            # ... and then its own pictures, two calls late, in decoding order


def test_a_plain_sequence_lags_by_what_waited_and_no_more():
    """... behind an old sequence that ends with ONE picture waiting where two might: everything that waited becomes ready at once, so the sequence that does not
    reorder runs one call late, not as many as the old sequence's reorder count"""
    assert calls(([(0, True)], 2), ([(k, k == 0) for k in range(5)], 0)) == [None, 1, 2, 3, 4, 5]
